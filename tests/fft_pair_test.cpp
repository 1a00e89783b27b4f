// Host-side run of the pair form's lane program (dc_tts_amd/csrc/fft_wave.h: the passes + fw_pair_split / fw_pair_merge), 64 "lanes" one after the other:
// two real frames -> one forward transform -> split into two spectra; two Hermitian spectra (the split ones, re-scaled per bin) -> merge -> one inverse
// transform -> two real frames.  Prints, for (a, b random) and (a random, b all zeros): max abs error of spectrum A, of B, of the two round trips (against a
// double-precision DFT), and the largest |A[k] - conj A[N-k]| + |B[k] - conj B[N-k]| of the split, which must be exactly 0.  Run by tests/test_fft_pair.py.
#include <cmath>
#include <complex>
#include <cstdio>
#include <vector>

#include "../dc_tts_amd/csrc/fft_wave.h"

using namespace dctts;
typedef std::complex<double> cd;
static float2 v[64][16];
static std::vector<float2> w(FW_N), ex(FW_EX);

template <bool INV> static void passes() {
  for (int l = 0; l < 64; ++l) fw_passA_store<INV>(v[l], ex.data(), l);
  for (int l = 0; l < 64; ++l) fw_passB_load<INV>(v[l], ex.data(), l, w.data());
  for (int l = 0; l < 64; ++l) fw_passB_store(v[l], ex.data(), l);
  for (int l = 0; l < 64; ++l) fw_passC_load<INV>(v[l], ex.data(), l, w.data());
}
// sum_n x[n] g(n) e^{sign 2 pi i k n / N}, g(n) = g0 + g1 min(n, N - n)
static cd dft(const std::vector<cd>& x, int k, double sign, double g0, double g1) {
  cd acc = 0;
  for (int n = 0; n < FW_N; ++n) acc += x[n] * (g0 + g1 * std::min(n, FW_N - n)) * std::polar(1.0, sign * 2.0 * M_PI * (double)((long)k * n % FW_N) / FW_N);
  return acc;
}

int main() {
  for (int m = 0; m < FW_N; ++m) w[m] = make_float2((float)std::cos(2.0 * M_PI * m / FW_N), (float)-std::sin(2.0 * M_PI * m / FW_N));
  unsigned s = 2468u;
  auto rnd = [&]() { s = s * 1664525u + 1013904223u; return (float)((s >> 8) & 0xffff) / 32768.0f - 1.0f; };
  for (int zero_b = 0; zero_b < 2; ++zero_b) {
    std::vector<cd> a(FW_N), b(FW_N), RA(FW_N), RB(FW_N);
    for (int n = 0; n < FW_N; ++n) { a[n] = rnd(); b[n] = zero_b ? 0.f : rnd(); }
    for (int k = 0; k < FW_N; ++k) { RA[k] = dft(a, k, -1, 1, 0); RB[k] = dft(b, k, -1, 1, 0); }
    for (int l = 0; l < 64; ++l) for (int q = 0; q < 16; ++q) v[l][q] = make_float2((float)a[l + 64 * q].real(), (float)b[l + 64 * q].real());      // the load
    passes<false>();
    // the kernels' exchange: every lane stores its 16 values, lane 0 also Z[N] = Z[0]; the partner of k = l + 64 r is at fw_base(64 - l) + 68 (15 - r)
    for (int l = 0; l < 64; ++l) for (int r = 0; r < 16; ++r) ex[fw_base(l) + 68 * r] = v[l][r];
    ex[FW_N + FW_N / 16] = v[0][0];
    double e[5] = {0, 0, 0, 0, 0};
    std::vector<float2> A(FW_N), B(FW_N);
    for (int l = 0; l < 64; ++l) for (int r = 0; r < 16; ++r) {
      const int k = l + 64 * r, kk = std::min(k, FW_N - k);
      fw_pair_split(v[l][r], ex[fw_base(64 - l) + 68 * (15 - r)], A[k], B[k]);
      e[0] = std::fmax(e[0], std::abs(RA[k] - cd(A[k].x, A[k].y)));
      e[1] = std::fmax(e[1], std::abs(RB[k] - cd(B[k].x, B[k].y)));
      const float ga = 1.0f + 0.001f * kk, gb = 2.0f - 0.002f * kk;          // two other Hermitian spectra: each lane scales its own bins
      v[l][r] = fw_pair_merge(make_float2(ga * A[k].x, ga * A[k].y), make_float2(gb * B[k].x, gb * B[k].y));
    }
    for (int k = 1; k < FW_N; ++k)          // the lane that owns N - k got the conjugates bit for bit: what lets the kernel skip a second exchange
      e[4] = std::fmax(e[4], std::fabs(A[k].x - A[FW_N - k].x) + std::fabs(A[k].y + A[FW_N - k].y) + std::fabs(B[k].x - B[FW_N - k].x) + std::fabs(B[k].y + B[FW_N - k].y));
    passes<true>();
    for (int n = 0; n < FW_N; n += 5) {
      const float2 z = v[n & 63][n >> 6];
      e[2] = std::fmax(e[2], std::abs(dft(RA, n, 1, (double)1.0f, (double)0.001f) - (double)z.x) / FW_N);
      e[3] = std::fmax(e[3], std::abs(dft(RB, n, 1, (double)2.0f, -(double)0.002f) - (double)z.y) / FW_N);
    }
    std::printf("%.3e %.3e %.3e %.3e %.3e\n", e[0], e[1], e[2], e[3], e[4]);
  }
  return 0;
}
