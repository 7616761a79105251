// BiLSTM text model (the reference's Keras fast path: model_training/train_lstm_text_model.py:96-120,
// inference/text_lstm_inference.py): Embedding [10000,128] -> Bidirectional(LSTM 128, sequences) ->
// Bidirectional(LSTM 64) -> Dense 128 relu -> Dense 64 relu -> Dense 7 softmax, all fp32.
//
// The input projections x.W + b are hoisted out of the recurrences. Layer 1's is a table
// Emb.W + b [10000][1024] (forward gates | backward gates) built once at creation and gathered per
// token by the recurrent kernel itself; layer 2's is one fp32 GEMM (gemm_f32.hip) over all B.L tokens
// and both directions. What remains per step is h.U, the gates and the state update:
//
// lstm_seq_kernel<UNITS, R>: one workgroup of 4 UNITS lanes walks all L steps of R rows of one
// direction; nothing is shared between workgroups. Lane (n, q) = (unit, quarter of K) holds
// U[q KQ .. q KQ + KQ - 1][gate 0..3][n] in registers for the whole launch (UNITS = 128: 128 VGPRs a
// lane, 8 waves, the whole 256 KB of U on chip; UNITS = 64: 64 VGPRs, 4 waves). Per step a lane reads
// its quarter of every row's h from LDS (the same address across a wave's lanes of one q: a
// broadcast), accumulates the four partial gate sums of every row in one ascending fmaf chain each,
// and the quad's four partial sums are added by two DPP steps, after which the four gates of unit n
// sit in every lane of the quad. Lane q then finishes row q (gates, c in a register, h), writes h
// into the other LDS buffer and (layer 1) the output sequence; one barrier ends the step. Every
// row's arithmetic is the same instruction sequence at every R and every position in the batch, so
// a row's bits depend on nothing but its own tokens.
#include "../../include/mec.h"

#include <algorithm>

#include "block_ops.h"
#include "models.h"

namespace mec {

namespace {

constexpr int kLstmIdsL = 128;  // longest sequence whose ids a workgroup stages (the model's L)

struct LstmSeq {
  const float* xz;     // gate pre-activations x.W + b (columns i | f | c | o per direction), rows ld floats apart
  const int32_t* ids;  // null: token (b, t) reads row b L + t of xz; else row clamp(ids[b L + t], 0, V - 1) (a projected table)
  int V;
  long long ld;
  const float* U[2];  // per direction: recurrent kernel [UNITS][4 UNITS]
  int xoff[2];        // the direction's first gate column within an xz row
  int reverse[2];     // the direction walks t = L - 1 .. 0 (outputs stay in time order)
  float* y;           // [B, L, ldy] output sequence or null; the direction's h at columns yoff ..
  long long ldy;
  int yoff[2];
  float* hl;          // [B, ldh] last h or null; the direction's at columns hoff ..
  long long ldh;
  int hoff[2];
  int B, L;
};

__device__ __forceinline__ float quad_sum(float v) {
  // quad_perm [1,0,3,2] then [2,3,0,1]: every lane of the quad ends with the same bits
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, true));
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xF, 0xF, true));
  return v;
}

__device__ __forceinline__ float lstm_sigmoid(float x) {
  return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(x * -1.44269504088896341f));
}

__device__ __forceinline__ float lstm_tanh(float x) {
  const float e = __builtin_amdgcn_exp2f(__builtin_fabsf(x) * -2.88539008177792681f);  // exp(-2|x|) in (0, 1]
  return __builtin_copysignf((1.0f - e) * __builtin_amdgcn_rcpf(1.0f + e), x);
}

template <int UNITS, int R>
__global__ __launch_bounds__(4 * UNITS) void lstm_seq_kernel(const LstmSeq p) {
  constexpr int KQ = UNITS / 4;  // k per lane
  constexpr int HP = KQ + 4;     // LDS floats per quarter of h: the four quarters a wave reads start in different banks
  __shared__ __attribute__((aligned(16))) float hbuf[2][R][4 * HP];
  __shared__ int sid[R][kLstmIdsL];
  const int tid = threadIdx.x, n = tid >> 2, q = tid & 3;
  const int d = blockIdx.y, b0 = blockIdx.x * R, L = p.L;
  const bool rev = p.reverse[d] != 0;

  float w[4][KQ];
  {
    const float* U = p.U[d] + (size_t)(q * KQ) * (4 * UNITS) + n;
#pragma unroll
    for (int k = 0; k < KQ; ++k)
#pragma unroll
      for (int g = 0; g < 4; ++g) w[g][k] = U[(size_t)k * (4 * UNITS) + g * UNITS];
  }

  // the row this lane finishes; lanes q >= R, and rows past the batch, repeat a row and store nothing
  const int rq = q < R ? q : R - 1;
  const int b = min(b0 + rq, p.B - 1);
  const bool own = q < R && b0 + q < p.B;
  if (p.ids) {
    for (int idx = tid; idx < R * L; idx += 4 * UNITS) {
      const int r = idx / L, t = idx - r * L;
      const int id = p.ids[(size_t)min(b0 + r, p.B - 1) * L + t];
      sid[r][t] = min(max(id, 0), p.V - 1);
    }
  }
  for (int idx = tid; idx < R * 4 * HP; idx += 4 * UNITS) (&hbuf[0][0][0])[idx] = 0.f;
  __syncthreads();

  const float* xbase = p.xz + p.xoff[d] + n;
  auto xrow = [&](int t) {
    const long long row = p.ids ? (long long)sid[rq][t] : (long long)b * L + t;
    return xbase + row * p.ld;
  };
  float xg[4];
  {
    const float* x = xrow(rev ? L - 1 : 0);
#pragma unroll
    for (int g = 0; g < 4; ++g) xg[g] = x[g * UNITS];
    // landed before the loop: a load still pending at the loop head would make the compiler wait for
    // every vector-memory operation (vmcnt(0)) at the first use of xg in each step, mid-step
#pragma unroll
    for (int g = 0; g < 4; ++g) asm volatile("" : "+v"(xg[g]));
  }
  const int hslot = (n / KQ) * HP + (n % KQ);
  float c = 0.f, h = 0.f;
  for (int s = 0; s < L; ++s) {
    const int t = rev ? L - 1 - s : s;
    float xn[4] = {0.f, 0.f, 0.f, 0.f};
    if (s + 1 < L) {  // the next step's pre-activations: in flight under this step
      const float* x = xrow(rev ? t - 1 : t + 1);
#pragma unroll
      for (int g = 0; g < 4; ++g) xn[g] = x[g * UNITS];
    }
    float acc[R][4];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int g = 0; g < 4; ++g) acc[r][g] = 0.f;
    const float* hc = &hbuf[s & 1][0][q * HP];
#pragma unroll
    for (int kk = 0; kk < KQ / 4; ++kk) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const floatx4 hv = *reinterpret_cast<const floatx4*>(hc + r * 4 * HP + 4 * kk);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int g = 0; g < 4; ++g) acc[r][g] = __builtin_fmaf(hv[j], w[g][4 * kk + j], acc[r][g]);
      }
    }
    float z[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      z[g] = quad_sum(acc[0][g]);
#pragma unroll
      for (int r = 1; r < R; ++r) {
        const float v = quad_sum(acc[r][g]);
        z[g] = q == r ? v : z[g];
      }
      z[g] += xg[g];
    }
    const float gi = lstm_sigmoid(z[0]), gf = lstm_sigmoid(z[1]), gc = lstm_tanh(z[2]), go = lstm_sigmoid(z[3]);
    c = __builtin_fmaf(gf, c, gi * gc);
    h = go * lstm_tanh(c);
    if (q < R) hbuf[(s + 1) & 1][q][hslot] = h;
    // the prefetch has had the whole step to land; taking it here, ahead of the store, leaves only that
    // store in flight across the barrier
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      asm volatile("" : "+v"(xn[g]));
      xg[g] = xn[g];
    }
    if (own && p.y) p.y[((size_t)b * L + t) * p.ldy + p.yoff[d] + n] = h;
    __syncthreads();
  }
  if (own && p.hl) p.hl[(size_t)b * p.ldh + p.hoff[d] + n] = h;
}

template <int UNITS>
int launch_lstm_seq_u(const LstmSeq& p, int ndir, int rows, hipStream_t s) {
  const dim3 blk(4 * UNITS);
  switch (rows) {
    case 1: hipLaunchKernelGGL((lstm_seq_kernel<UNITS, 1>), dim3(p.B, ndir), blk, 0, s, p); break;
    case 2: hipLaunchKernelGGL((lstm_seq_kernel<UNITS, 2>), dim3((p.B + 1) / 2, ndir), blk, 0, s, p); break;
    default: hipLaunchKernelGGL((lstm_seq_kernel<UNITS, 4>), dim3((p.B + 3) / 4, ndir), blk, 0, s, p); break;
  }
  MEC_LAUNCH_CHECK();
  return 0;
}

int launch_lstm_seq(const LstmSeq& p, int units, int ndir, hipStream_t s) {
  MEC_REQUIRE(units == 64 || units == 128, "lstm_seq: units must be 64 or 128");
  MEC_REQUIRE(p.B > 0 && p.L >= 1, "lstm_seq: B > 0 and L >= 1");
  MEC_REQUIRE(!p.ids || p.L <= kLstmIdsL, "lstm_seq: gathered rows need L <= 128");
  const int rows = opt().lstm_rows;
  return units == 128 ? launch_lstm_seq_u<128>(p, ndir, rows, s) : launch_lstm_seq_u<64>(p, ndir, rows, s);
}

// Layer 1's projected table, once per handle: T[v][n] = b[n] + sum_k E[v][k] W[k][n] (one ascending
// fmaf chain), W [128][1024] = forward | backward kernels. Grid V, 1024 threads.
__global__ __launch_bounds__(1024) void lstm_table_kernel(const float* __restrict__ E, const float* __restrict__ W,
                                                          const float* __restrict__ bias, float* __restrict__ T) {
  __shared__ float e[128];
  const int v = blockIdx.x, n = threadIdx.x;
  if (n < 128) e[n] = E[(size_t)v * 128 + n];
  __syncthreads();
  float acc = 0.f;
#pragma unroll 16
  for (int k = 0; k < 128; ++k) acc = __builtin_fmaf(e[k], W[(size_t)k * 1024 + n], acc);
  T[(size_t)v * 1024 + n] = acc + bias[n];
}

// Dense 128 relu -> Dense 64 relu (feat) -> Dense 7 -> softmax; R rows per workgroup, 256 threads.
struct LstmHeadW {
  const float *w1, *b1, *w2, *b2, *w3, *b3;  // Keras kernels [in][out]
};
constexpr int kHeadR = 4;
__global__ __launch_bounds__(256) void lstm_head_kernel(LstmHeadW w, const float* __restrict__ X, int B,
                                                        float* __restrict__ feat, float* __restrict__ logits,
                                                        float* __restrict__ probs) {
  constexpr int R = kHeadR;
  __shared__ __attribute__((aligned(16))) float X0[R * 128], Y1[R * 128], Y2[R * 64], Z[R * 8], red[4096];
  const int tid = threadIdx.x, r0 = blockIdx.x * R, nr = min(R, B - r0);
  for (int idx = tid; idx < R * 128; idx += 256) {
    const int r = idx >> 7;
    X0[idx] = r < nr ? X[(size_t)(r0 + r) * 128 + (idx & 127)] : 0.f;
  }
  __syncthreads();
  block_linear<R>(X0, 128, 128, w.w1, 128, w.b1, 128, Y1, 128, red, BACT_RELU);
  block_linear<R>(Y1, 128, 128, w.w2, 64, w.b2, 64, Y2, 64, red, BACT_RELU);
  if (feat)
    for (int idx = tid; idx < nr * 64; idx += 256) feat[(size_t)r0 * 64 + idx] = Y2[idx];
  block_linear<R>(Y2, 64, 64, w.w3, 7, w.b3, 7, Z, 8, red, BACT_NONE);
  if (logits)
    for (int idx = tid; idx < nr * 7; idx += 256) logits[(size_t)r0 * 7 + idx] = Z[(idx / 7) * 8 + idx % 7];
  __syncthreads();
  block_softmax_small<R>(Z, 8, 7, nullptr, 0);
  if (probs)
    for (int idx = tid; idx < nr * 7; idx += 256) probs[(size_t)r0 * 7 + idx] = Z[(idx / 7) * 8 + idx % 7];
}

}  // namespace

int lstm_seq_f32(const float* xz, const float* U, int B, int L, int units, int reverse, float* y_seq, float* h_last,
                 hipStream_t s) {
  MEC_REQUIRE(units == 64 || units == 128, "lstm_seq: units must be 64 or 128");
  MEC_REQUIRE(L >= 1, "lstm_seq: L >= 1");
  MEC_REQUIRE(B >= 0, "lstm_seq: B < 0");
  MEC_REQUIRE(reverse == 0 || reverse == 1, "lstm_seq: reverse must be 0 or 1");
  if (B == 0) return 0;
  MEC_REQUIRE(xz && U, "lstm_seq: null operand");
  MEC_REQUIRE(y_seq || h_last, "lstm_seq: no output");
  LstmSeq p{};
  p.xz = xz; p.ld = 4 * units; p.U[0] = U; p.reverse[0] = reverse;
  p.y = y_seq; p.ldy = units; p.hl = h_last; p.ldh = units; p.B = B; p.L = L;
  return launch_lstm_seq(p, units, 1, s);
}

int LstmTextModel::create(const float* blob, size_t n) {
  constexpr int V = kVocab, E = 128, U1 = 128, U2 = 64;
  BlobReader rd(blob, n);
  const float* emb = rd.take((size_t)V * E);
  struct Dir { const float *k, *u, *b; };
  Dir l1[2], l2[2];
  for (auto& d : l1) { d.k = rd.take((size_t)E * 4 * U1); d.u = rd.take((size_t)U1 * 4 * U1); d.b = rd.take(4 * U1); }
  for (auto& d : l2) { d.k = rd.take((size_t)2 * U1 * 4 * U2); d.u = rd.take((size_t)U2 * 4 * U2); d.b = rd.take(4 * U2); }
  const float* dw[3];
  const float* db[3];
  const int din[3] = {2 * U2, 128, 64}, dout[3] = {128, 64, 7};
  for (int i = 0; i < 3; ++i) { dw[i] = rd.take((size_t)din[i] * dout[i]); db[i] = rd.take(dout[i]); }
  MEC_REQUIRE(rd.ok && rd.off == n, "text_lstm blob size mismatch");

  std::vector<float> h;
  auto put = [&](const float* src, size_t cnt) {
    const size_t o = h.size();
    h.insert(h.end(), src, src + cnt);
    return o;
  };
  off_table = h.size();
  h.resize((size_t)V * 8 * U1);  // filled on the device below
  for (int d = 0; d < 2; ++d) off_u1[d] = put(l1[d].u, (size_t)U1 * 4 * U1);
  // layer 2's projection as the fp32 engine's B operand [N = 512][K = 256]: rows = forward | backward gate columns
  off_w2 = h.size();
  h.resize(off_w2 + (size_t)8 * U2 * 2 * U1);
  for (int d = 0; d < 2; ++d)
    for (int nn = 0; nn < 4 * U2; ++nn)
      for (int k = 0; k < 2 * U1; ++k) h[off_w2 + (size_t)(d * 4 * U2 + nn) * 2 * U1 + k] = l2[d].k[(size_t)k * 4 * U2 + nn];
  off_b2 = put(l2[0].b, 4 * U2);
  put(l2[1].b, 4 * U2);
  for (int d = 0; d < 2; ++d) off_u2[d] = put(l2[d].u, (size_t)U2 * 4 * U2);
  for (int i = 0; i < 3; ++i) { off_dw[i] = put(dw[i], (size_t)din[i] * dout[i]); off_db[i] = put(db[i], dout[i]); }
  MEC_TRY(upload(w, h.data(), h.size() * sizeof(float)));

  // the projected table: Emb . [W_fwd | W_bwd] + [b_fwd | b_bwd]
  std::vector<float> t((size_t)V * E + (size_t)E * 8 * U1 + 8 * U1);
  std::copy(emb, emb + (size_t)V * E, t.begin());
  float* wc = t.data() + (size_t)V * E;
  for (int k = 0; k < E; ++k)
    for (int d = 0; d < 2; ++d) std::copy(l1[d].k + (size_t)k * 4 * U1, l1[d].k + (size_t)(k + 1) * 4 * U1, wc + (size_t)k * 8 * U1 + d * 4 * U1);
  float* bc = wc + (size_t)E * 8 * U1;
  for (int d = 0; d < 2; ++d) std::copy(l1[d].b, l1[d].b + 4 * U1, bc + d * 4 * U1);
  DevBuf tmp;
  MEC_TRY(upload(tmp, t.data(), t.size() * sizeof(float)));
  const float* td = tmp.as<float>();
  hipLaunchKernelGGL(lstm_table_kernel, dim3(V), dim3(1024), 0, nullptr, td, td + (size_t)V * E,
                     td + (size_t)V * E + (size_t)E * 8 * U1, w.as<float>() + off_table);
  MEC_LAUNCH_CHECK();
  MEC_HIP(hipDeviceSynchronize());  // tmp is freed on return
  return 0;
}

int LstmTextModel::forward(const int32_t* ids, int B, int L, float* feat, float* logits, float* probs, hipStream_t s) {
  constexpr int U1 = 128, U2 = 64;
  MEC_REQUIRE(B >= 0, "text_lstm: B < 0");
  MEC_REQUIRE(L == 128, "text_lstm: L must be 128 (pad_sequences maxlen = Config.MAX_TEXT_LENGTH)");
  if (B == 0) return 0;
  MEC_REQUIRE(ids && probs, "text_lstm: null pointer");
  const float* P = w.as<float>();
  const size_t M = (size_t)B * L;
  float *y1, *xz2, *h2;
  MEC_TRY(carve(ws, [&](Carver& c) {
    y1 = c.take<float>(M * 2 * U1);
    xz2 = c.take<float>(M * 8 * U2);
    h2 = c.take<float>((size_t)B * 2 * U2);
  }));
  LstmSeq a{};
  a.xz = P + off_table; a.ids = ids; a.V = kVocab; a.ld = 8 * U1; a.B = B; a.L = L;
  a.y = y1; a.ldy = 2 * U1;
  for (int d = 0; d < 2; ++d) { a.U[d] = P + off_u1[d]; a.xoff[d] = d * 4 * U1; a.reverse[d] = d; a.yoff[d] = d * U1; }
  MEC_TRY(prof.begin(TAG_LSTM_REC1, s));
  MEC_TRY(launch_lstm_seq(a, U1, 2, s));
  MEC_TRY(prof.end(TAG_LSTM_REC1, s));

  GemmParams g;
  g.A = y1; g.B32 = P + off_w2; g.bias = P + off_b2; g.C32 = xz2; g.M = (int)M; g.N = 8 * U2; g.K = 2 * U1;
  MEC_TRY(prof.begin(TAG_LSTM_PROJ, s));
  MEC_TRY(launch_gemm_f32(g, s, nullptr, TAG_NONE));
  MEC_TRY(prof.end(TAG_LSTM_PROJ, s));

  LstmSeq c{};
  c.xz = xz2; c.ld = 8 * U2; c.B = B; c.L = L; c.hl = h2; c.ldh = 2 * U2;
  for (int d = 0; d < 2; ++d) { c.U[d] = P + off_u2[d]; c.xoff[d] = d * 4 * U2; c.reverse[d] = d; c.hoff[d] = d * U2; }
  MEC_TRY(prof.begin(TAG_LSTM_REC2, s));
  MEC_TRY(launch_lstm_seq(c, U2, 2, s));
  MEC_TRY(prof.end(TAG_LSTM_REC2, s));

  const LstmHeadW hw{P + off_dw[0], P + off_db[0], P + off_dw[1], P + off_db[1], P + off_dw[2], P + off_db[2]};
  MEC_TRY(prof.begin(TAG_LSTM_HEAD, s));
  hipLaunchKernelGGL(lstm_head_kernel, dim3((B + kHeadR - 1) / kHeadR), dim3(256), 0, s, hw, h2, B, feat, logits, probs);
  MEC_LAUNCH_CHECK();
  MEC_TRY(prof.end(TAG_LSTM_HEAD, s));
  return 0;
}

}  // namespace mec
