"""Float64 reference of BERT's self-attention (128 tokens, 12 heads of 64), the error bound its HIP
kernels are held to, the input cases of tests/test_gpu_attention.py and the hi / lo plane helpers of
the fp32x3 path. Test infrastructure only; checked on the CPU by tests/test_attn_ref.py.

Reference. O = softmax(Q K^T / 8 + bias) V per (sequence, head), written from the definition with a
loop over sequences and heads and no layout tricks. bias is 0 for a key the query may see and
finfo(f32).min otherwise: in fp32 finfo.min + s == finfo.min for every |s| < 2^103, so a masked
key's probability is exactly 0 next to any valid key -- and a query with NO valid key sees 128 equal
scores, i.e. the uniform mean of all 128 V rows (what transformers computes, and the kernels too).

Bound. Per output element (query i, feature d), with u = 2^-24 and, from the reference,
  pav  = sum_j p_j |v_jd|                    A  = max over the query's valid keys of sum_c |q_ic| |k_jc| / 8
  pdav = sum_j p_j (m - s_j) |v_jd|          ed = sum_j p_j (m - s_j)          (m = the row's max score)
the kernels owe |err| <= (e^(2 ds) - 1 + e_p + e_o) pav + e_x + floor:
  ds    the score error. Every kernel sums the 64 products of a score into one fp32 accumulator (f16 x f16
        products are exact in fp32, the fp32 MFMA is an fma chain): 64 u A. fp32x3 drops the lo.lo
        product, |q_lo| |k_lo| <= 2^-22 |q| |k|: (64 u + 2^-22) A. Its hi.lo and lo.hi products go into
        the same accumulator; their 128 further additions are NOT counted: only the 64 hi.hi accumulations
        are, the stricter choice (192 u A would be the rigorous worst case). The 1/8 (and qks) is a power of two and the bias 0: exact. A score error of ds
        on every key moves every probability by a factor within e^(+-2 ds).
  e_x   exp and the normalization: the argument s_j - m is rounded once (u |s_j - m|), the f16 kernel
        multiplies by log2(e) (its rounding and the constant's: 2 u |s_j - m| more), exp itself is good to
        1 ulp (2 u); the 128-term sum, the reciprocal and p / sum add 130 u, and the sum carries the
        p-weighted mean of the per-term errors:  c u (pdav + ed pav) + 134 u pav, c = 3 (f16) or 1.
  e_p   P as an MFMA operand: f16 2^-11; fp32x3 the hi / lo split's residual 2^-22; fp32 0.
  e_o   O: 128 fp32 additions (128 u), plus f16: the f16 result 2^-11; fp32x3: the dropped p_lo v_lo
        2^-22 and the output planes' residual 2^-22.
  floor f16 only: a probability below f16's subnormal step is off by up to 2^-25 absolutely, on each of the
        128 keys: 128 2^-25 max_j |v_jd| over the query's valid keys (a masked key's p is exactly 0), and the
        f16 output's own subnormal step 2^-25. fp32x3: the lo output plane's subnormal step, 2^-25 2^-s_v.
Where this departs from the plain form (e^(2 ds) - 1 + e_p + e_o) pav + an f16-only floor of
128 2^-25 max |v|, and why -- each is a term of the derivation, none was fitted to a kernel's output:
  1. fp32x3 has a floor too, 2^-25 2^-s_v: where |O 2^s_v| < 2^-3 the lo output plane is an f16 subnormal and
     its rounding is absolute, not relative to pav (the largest measured ratios sit exactly there).
  2. The f16 floor carries 2^-25 more: the f16 output's own subnormal half step for |O| < 2^-14.
  3. fp32x3's e_o is 2^-21, not 2^-22: the P V product drops p_lo v_lo as the scores drop q_lo k_lo.
  4. exp's error is the separate term e_x, not a constant inside e_p: it grows with m - s_j, so it is weighted
     per key by p_j (m - s_j) instead of by the row's worst m - s_j, which is tighter for the far keys.
  5. The f16 floor's max |v| runs over the query's valid keys only (a masked key's p is exactly 0): tighter.
The mutations of tests/test_attn_ref.py exceed the bound by factors of 1e3 to 1e8, so none of this costs
sensitivity. No factor is tuned: tests/test_gpu_attention.py prints max(err / bound) per case and lists the values.
"""
import numpy as np
import torch

from mec import x3pair

L, HEADS, DH, H = 128, 12, 64, 768
U = 2.0 ** -24
PRECS = ('f16', 'fp32', 'x3')


# ------------------------------------------------------------------ reference
def valid_from_mask(mask):
    """int mask [R, 128] -> valid[r, i, j]: query i of row r may see key j (mask[r, j] != 0)."""
    m = np.asarray(mask) != 0
    return np.broadcast_to(m[:, None, :], (m.shape[0], L, L)).copy()


def valid_from_segments(seg):
    """uint8 segment ids [R, 128] -> valid[r, i, j]: key j is in query i's own segment."""
    s = np.asarray(seg).astype(np.int64)
    return s[:, :, None] == s[:, None, :]


def attention(q, k, v, valid, mutate=None):
    """q, k, v [R, 12, 128, 64] (any float type, taken as float64), valid [R, 128, 128] bool ->
    dict of float64 arrays: o, pav, pdav [R, 12, 128, 64]; A, ed [R, 12, 128]; vmax [R, 12, 128, 64]
    (max |v_jd| over the query's valid keys). `mutate` (tests/test_attn_ref.py): one of MUTATIONS, a way
    a kernel goes wrong, applied to o only."""
    q, k, v = (np.asarray(t, np.float64) for t in (q, k, v))
    R = q.shape[0]
    out = {n: np.zeros((R, HEADS, L, DH)) for n in ('o', 'pav', 'pdav', 'vmax')}
    out.update({n: np.zeros((R, HEADS, L)) for n in ('A', 'ed')})
    for r in range(R):
        ok = valid[r].copy()
        none = ~ok.any(axis=1)
        ok[none] = True  # no valid key: 128 equal scores (finfo.min absorbs them all), uniform attention
        for h in range(HEADS):
            s = q[r, h] @ k[r, h].T / 8.0
            s[none] = 0.0
            a = np.abs(q[r, h]) @ np.abs(k[r, h]).T / 8.0
            a[none] = 0.0
            sm = np.where(ok, s, -np.inf)
            m = sm.max(axis=1, keepdims=True)
            e = np.exp(sm - m)
            p = e / e.sum(axis=1, keepdims=True)
            dist = np.where(ok, m - s, 0.0)
            av = np.abs(v[r, h])
            out['o'][r, h] = p @ v[r, h]
            out['pav'][r, h] = p @ av
            out['pdav'][r, h] = (p * dist) @ av
            out['ed'][r, h] = (p * dist).sum(axis=1)
            out['A'][r, h] = np.where(ok, a, 0.0).max(axis=1)
            out['vmax'][r, h] = (ok[:, :, None] * av[None, :, :]).max(axis=1)
            if mutate is not None:
                out['o'][r, h] = _mutated(mutate, s, ok, valid[r], v[r], h)
    return out


MUTATIONS = ('swap_keys', 'leak_masked_key', 'half_max', 'next_head_v')


def _mutated(kind, s, ok, valid_r, v_r, h):
    """The head's output with one kernel bug:
    swap_keys        P's keys 4..7 and 8..11 exchanged while V keeps its order (a score-tile / V^T mismatch)
    leak_masked_key  the first masked key of each query counts (for a query with none: no change)
    half_max         the two 64-key halves a lane pair holds (key bit 2 clear / set) each subtract their OWN
                     max and share one sum: the cross-half max exchange missing
    next_head_v      head h multiplies head h + 1's V"""
    ok = ok.copy()
    if kind == 'leak_masked_key':
        for i in np.flatnonzero((~valid_r).any(axis=1) & valid_r.any(axis=1)):
            ok[i, np.flatnonzero(~valid_r[i])[0]] = True
    sm = np.where(ok, s, -np.inf)
    if kind == 'half_max':
        half = (np.arange(L) >> 2) & 1
        m = np.empty_like(sm)
        for b in (0, 1):
            mb = sm[:, half == b].max(axis=1, keepdims=True)
            m[:, half == b] = np.where(np.isfinite(mb), mb, 0.0)
    else:
        m = sm.max(axis=1, keepdims=True)
    with np.errstate(over='ignore', invalid='ignore'):
        e = np.exp(sm - m)
        p = e / e.sum(axis=1, keepdims=True)
    if kind == 'swap_keys':
        perm = np.arange(L)
        perm[4:8], perm[8:12] = np.arange(8, 12), np.arange(4, 8)
        p = p[:, perm]
    return p @ v_r[(h + 1) % HEADS if kind == 'next_head_v' else h]


# ------------------------------------------------------------------ bound
def bound(ref, prec, s_v=0):
    """The bound of the module docstring per output element [R, 12, 128, 64]; prec in PRECS."""
    A = ref['A'][..., None]
    pav = ref['pav']
    c = 3.0 if prec == 'f16' else 1.0
    ds = (64 * U + (2.0 ** -22 if prec == 'x3' else 0.0)) * A
    e_p = {'f16': 2.0 ** -11, 'fp32': 0.0, 'x3': 2.0 ** -22}[prec]
    e_o = 128 * U + {'f16': 2.0 ** -11, 'fp32': 0.0, 'x3': 2.0 ** -21}[prec]
    e_x = c * U * (ref['pdav'] + ref['ed'][..., None] * pav) + 134 * U * pav
    floor = {'f16': 128 * 2.0 ** -25 * ref['vmax'] + 2.0 ** -25, 'fp32': 0.0, 'x3': 2.0 ** (-25 - s_v)}[prec]
    return (np.expm1(2 * ds) + e_p + e_o) * pav + e_x + floor


def ratio(got, ref, prec, s_v=0):
    """max(err / bound) over every output element; inf where `got` is not finite."""
    got = np.asarray(got, np.float64)
    r = np.abs(got - ref['o']) / bound(ref, prec, s_v)
    return float(np.where(np.isfinite(got), r, np.inf).max())


# ------------------------------------------------------------------ layouts
def to_rows(t):
    """[R, 12, 128, 64] -> [R * 128, 768] (token rows, head-major features)."""
    return np.ascontiguousarray(np.asarray(t).transpose(0, 2, 1, 3)).reshape(-1, H)


def from_rows(t):
    """[R * 128, 768] -> [R, 12, 128, 64]."""
    t = np.asarray(t)
    return t.reshape(-1, L, HEADS, DH).transpose(0, 2, 1, 3)


def split(x, s=0):
    """fp32 x -> f16 planes (hi, lo) of x 2^s: hi = f16(x 2^s), lo = f16(x 2^s - hi)."""
    y = np.ldexp(np.asarray(x, np.float32), s)
    hi = y.astype(np.float16)
    return hi, (y - hi.astype(np.float32)).astype(np.float16)


def value(hi, lo, s=0):
    """The float64 value planes at 2^s stand for."""
    return np.ldexp(np.asarray(hi, np.float64) + np.asarray(lo, np.float64), -s)


def planar(hi, lo, pad=192):
    """One f16 torch buffer holding the hi plane and, lo_off elements on, the lo plane; returns (buffer, lo_off).
    hi / lo: 2-D numpy f16 arrays."""
    lo_off = hi.size + pad
    buf = torch.zeros(lo_off + hi.size, dtype=torch.float16)
    buf[:hi.size] = torch.from_numpy(np.ascontiguousarray(hi)).reshape(-1)
    buf[lo_off:] = torch.from_numpy(np.ascontiguousarray(lo)).reshape(-1)
    return buf, lo_off


def paired(hi, lo):
    """The paired [rows, 2K] torch tensor of 2-D numpy f16 planes (mec/x3pair.py)."""
    return x3pair.pair(torch.from_numpy(np.ascontiguousarray(hi)), torch.from_numpy(np.ascontiguousarray(lo)))


# ------------------------------------------------------------------ cases
def _f16(x):
    return np.asarray(x, np.float32).astype(np.float16).astype(np.float32)


def _all_valid(R):
    return np.ones((R, L), np.int32)


def case_random(R, score_std, seed):
    """Q, K ~ N(0, sigma^2) with sigma^2 = score_std (the scores' std is sigma^2 sqrt(64) / 8), V ~ N(0, 1)."""
    g = np.random.default_rng(seed)
    sig = np.sqrt(score_std)
    q, k = (g.standard_normal((R, HEADS, L, DH)).astype(np.float32) * np.float32(sig) for _ in range(2))
    return dict(q=q, k=k, v=g.standard_normal((R, HEADS, L, DH)).astype(np.float32), mask=_all_valid(R))


def case_diffuse(R=2, seed=1):
    return case_random(R, 0.3, seed)


def case_peaked(R=3, seed=2):
    return case_random(R, 12.0, seed)


def case_planted(R=3, seed=3):
    """Per (sequence, head) a permutation pi: Q row i = 3 u_i and K row pi(i) = 3 u_i with u_i random +-1
    vectors, so query i's score on key pi(i) is 9 * 64 / 8 = 72 and every other one is 9/8 x a sum of 64
    random signs (std 9): O[i] = V[pi(i)] to the bound. Returns pi too ([R, 12, 128])."""
    g = np.random.default_rng(seed)
    u = g.integers(0, 2, (R, HEADS, L, DH)).astype(np.float32) * 2 - 1
    pi = np.stack([np.stack([g.permutation(L) for _ in range(HEADS)]) for _ in range(R)])
    k = np.empty_like(u)
    for r in range(R):
        for h in range(HEADS):
            k[r, h, pi[r, h]] = 3 * u[r, h]
    return dict(q=3 * u, k=k, v=g.standard_normal((R, HEADS, L, DH)).astype(np.float32), mask=_all_valid(R), pi=pi)


def case_offset(R=2, seed=4):
    """Feature 63 of every key is 40 and of every query +40 (even sequences) or -40 (odd): every score of a
    row carries a common +-200; the other 63 features give a spread of std 2."""
    c = case_random(R, 2.0 * 8 / np.sqrt(63), seed)
    c['k'][..., 63] = 40.0
    c['q'][..., 63] = np.where(np.arange(R) % 2 == 0, 40.0, -40.0)[:, None, None].astype(np.float32)
    return c


PREFIX_LENS = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128)


def _adversarial(g, R, seg):
    """Q, K, V [R, 12, 128, 64] where the keys a query must NOT see carry its row's largest raw scores and
    V = 1000. seg [R, 128]: token t belongs to group seg[r, t]; a query sees its own group only. Query i is
    noise + mu_g(i) with mu_g = 8 e_(g % 64) (so |mu|^2 = 64 and the groups' directions are orthogonal);
    key j is noise + 4 (sum of the row's other groups' mu): its raw score on a query of another group is about
    4 * 64 / 8 = 32 above that query's scores on its own group. V row j is noise + 1000 in feature
    g(j) % 64, so a leak from group g shows in a feature where the query's own group holds only noise."""
    q, k, v = (g.standard_normal((R, HEADS, L, DH)).astype(np.float32) for _ in range(3))
    for r in range(R):
        present = np.unique(seg[r])
        for t in range(L):
            own = int(seg[r, t])
            q[r, :, t, own % DH] += 8.0
            for o in present:
                if o != own:
                    k[r, :, t, int(o) % DH] += 32.0
            v[r, :, t, own % DH] += 1000.0
    return q, k, v


def case_masks(seed=5):
    """15 sequences, one mask each: the prefix lengths, Bernoulli(0.5) holes, only key 127, only key 0, key 0
    masked, all masked. The masked keys are adversarial (_adversarial with groups valid = 0, masked = 1: the
    masked keys' K is 4 x the valid queries' common part, their V 1000); a masked QUERY's row is compared too."""
    g = np.random.default_rng(seed)
    R = len(PREFIX_LENS) + 5
    mask = np.zeros((R, L), np.int32)
    for r, n in enumerate(PREFIX_LENS):
        mask[r, :n] = 1
    r = len(PREFIX_LENS)
    mask[r] = g.integers(0, 2, L)
    mask[r + 1, 127] = 1
    mask[r + 2, 0] = 1
    mask[r + 3, 1:] = 1
    q, k, v = _adversarial(g, R, 1 - mask)
    return dict(q=q, k=k, v=v, mask=mask)


SEGMENT_ROWS = ([128], [2] * 64, [1, 127], [60, 60, 8], [3])


def case_packed(seed=6):
    """Packed rows: the sentences of SEGMENT_ROWS back to back, the rest of a row segment 255 (the pack
    kernel's id for unused slots, a segment of their own). Every key is adversarial for the other segments'
    queries (_adversarial). cidx: the [CLS]-only form's samples, slots 0, 60 and 120 of rows listed out of
    order (so sample b's row is not b)."""
    g = np.random.default_rng(seed)
    R = len(SEGMENT_ROWS)
    seg = np.full((R, L), 255, np.uint8)
    for r, lens in enumerate(SEGMENT_ROWS):
        t = 0
        for i, n in enumerate(lens):
            seg[r, t:t + n] = i
            t += n
    q, k, v = _adversarial(g, R, seg)
    cidx = np.array([row * L + slot for row in (3, 1, 4, 0, 2) for slot in (0, 60, 120)], np.int32)
    return dict(q=q, k=k, v=v, seg=seg, cidx=cidx)


def valid_of(case):
    return valid_from_segments(case['seg']) if 'seg' in case else valid_from_mask(case['mask'])


def f16_exact(case):
    """The case with Q, K, V rounded to f16 (the f16 kernels' operands, which the reference then sees)."""
    return {**case, **{n: _f16(case[n]) for n in 'qkv'}}
