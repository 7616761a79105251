// The resampler of the audio front end (audio_load.hip), designed on the host: a polyphase Kaiser-windowed
// sinc from rate_in to rate_out, in float64. With g = gcd(rate_in, rate_out), up = rate_out / g,
// down = rate_in / g and M = max(up, down):
//   passband to 0.913 of the lower rate's Nyquist, stopband from 1.0 of it, design attenuation A = 125 dB
//   half = ceil((A - 7.95) / (2.285 * (1 - 0.913) * pi / M) / 2),  beta = 0.1102 * (A - 8.7)
//   fc   = (0.913 + 1) / 2 / M
//   h[n] = fc * sinc(fc * n) * kaiser(n),  n = -half .. half,  normalised to unit sum
// and output m of a signal x is sum_k up * h[half + m * down - k * up] * x[k]. This is the project's own
// filter, shaped after a high-quality resampler's published figures; it is not bit-compatible with any other.
// Plain C++ (no HIP), so it also compiles into a stand-alone host program (tools/resample_design_check.cpp,
// run under the address and undefined-behaviour sanitizers).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace mec {
namespace rs {

constexpr double kAtten = 125.0;
constexpr double kPass = 0.913;
constexpr double kPi = 3.14159265358979323846;
constexpr long long kMaxRate = 192000;
constexpr long long kMaxM = 8192;
constexpr long long kMaxTaps = 1ll << 21;
// floats of one workgroup's input window in LDS (audio_load.hip); the window of one output cycle must fit
constexpr long long kWindow = 16128;

struct Plan {
  int up = 1, down = 1, half = 0;  // half == 0: the identity plan (up == down == 1, no filter)
  long long taps() const { return half ? 2ll * half + 1 : 0; }
  // phase-major form: phase p = (m * down) mod up holds taps j = -L .. R, padded to an even J
  int L() const { return (int)((half + up - 1) / up); }
  int J() const {
    const int j = L() + half / up + 1;
    return j + (j & 1);
  }
};

inline long long gcd(long long a, long long b) {
  while (b) {
    const long long t = a % b;
    a = b;
    b = t;
  }
  return a;
}

// The plan of rate_in -> rate_out; false outside the domain (1 <= rate <= 192000, M <= 8192, at most 2^21
// taps, and one output cycle's input window, down + J samples, within kWindow).
inline bool plan(long long rate_in, long long rate_out, Plan* out) {
  if (rate_in < 1 || rate_in > kMaxRate || rate_out < 1 || rate_out > kMaxRate) return false;
  const long long g = gcd(rate_in, rate_out);
  const long long up = rate_out / g, down = rate_in / g, M = up > down ? up : down;
  if (M > kMaxM) return false;
  Plan p;
  p.up = (int)up;
  p.down = (int)down;
  if (M > 1) {
    const double width = 2.285 * (1.0 - kPass) * kPi / (double)M;
    const double half = std::ceil((kAtten - 7.95) / width / 2.0);
    if (2.0 * half + 1.0 > (double)kMaxTaps) return false;
    p.half = (int)half;
    if ((long long)p.down + p.J() > kWindow) return false;
  }
  if (out) *out = p;
  return true;
}

// Modified Bessel function I0 by its power series, sum ((x/2)^k / k!)^2; relative error near 1e-16 for the
// arguments a Kaiser window takes (0 <= x <= beta = 12.8).
inline double bessel_i0(double x) {
  const double q = 0.25 * x * x;
  double term = 1.0, sum = 1.0;
  for (int k = 1; k < 200; ++k) {
    term *= q / ((double)k * (double)k);
    sum += term;
    if (term < 1e-18 * sum) break;
  }
  return sum;
}

// h[0 .. 2 * half] of a non-identity plan, unit sum (Neumaier's compensated sum: a table has up to 2^21 taps).
inline void taps(const Plan& p, double* h) {
  const long long n = p.taps();
  const double M = (double)(p.up > p.down ? p.up : p.down);
  const double fc = (kPass + 1.0) / 2.0 / M;
  const double beta = 0.1102 * (kAtten - 8.7);
  const double i0b = bessel_i0(beta);
  for (long long i = 0; i < n; ++i) {
    const double t = (double)(i - p.half);
    const double a = kPi * fc * t;
    const double sinc = t == 0.0 ? 1.0 : std::sin(a) / a;
    const double r = t / (double)p.half;
    const double w = bessel_i0(beta * std::sqrt(std::fmax(0.0, 1.0 - r * r))) / i0b;
    h[i] = fc * sinc * w;
  }
  double sum = 0.0, comp = 0.0;
  for (long long i = 0; i < n; ++i) {
    const double t = sum + h[i];
    comp += std::fabs(sum) >= std::fabs(h[i]) ? (sum - t) + h[i] : (h[i] - t) + sum;
    sum = t;
  }
  const double total = sum + comp;
  for (long long i = 0; i < n; ++i) h[i] /= total;
}

// The phase-major table the kernel reads: g[p * J + jj] = up * h[half + p + (jj - L) * up], 0 off the ends,
// so that output m, with q = (m * down) / up and p = (m * down) mod up, is sum_jj g[p][jj] * x[q + L - jj].
inline void phase_major(const Plan& p, const double* h, double* g) {
  const int J = p.J(), L = p.L();
  for (int ph = 0; ph < p.up; ++ph)
    for (int jj = 0; jj < J; ++jj) {
      const long long at = (long long)p.half + ph + (long long)(jj - L) * p.up;
      g[(size_t)ph * J + jj] = at >= 0 && at <= 2ll * p.half ? (double)p.up * h[at] : 0.0;
    }
}

// The kernel's schedule for a plan (audio_load.hip): a workgroup owns G * cycles * up consecutive outputs, its
// lanes the cycles * up columns, each with G outputs cycles * up apart (the same phase), and stages
// G * cycles * down + J - 1 input samples. At least `threads` columns where the window allows, then as many
// outputs per lane (8, 4, 2 or 1) as keep the window within kWindow; plan() has checked that cycles = G = 1 fits.
inline void schedule(const Plan& p, int threads, int* cycles, int* G) {
  const long long room = kWindow - (p.J() - 1);
  long long n = (threads + p.up - 1) / p.up;
  if (n > room / p.down) n = room / p.down;
  if (n < 1) n = 1;
  int g = 8;
  while (g > 1 && g * n * p.down > room) g >>= 1;
  *cycles = (int)n;
  *G = g;
}

// librosa 0.10.0 resample's length, literally: int(np.ceil(frames * (float(rate_out) / rate_in))).
inline long long out_len(long long frames, long long rate_in, long long rate_out) {
  return (long long)std::ceil((double)frames * ((double)rate_out / (double)rate_in));
}

}  // namespace rs
}  // namespace mec
