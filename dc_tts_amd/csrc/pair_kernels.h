// pair_kernels.h -- the vocoder and the analysis direction at n_fft = 1024 (513 bins): ONE TRANSFORM CARRIES TWO ADJACENT FRAMES.
//
// vocoder_kernels.h / analysis_kernels.h pack one real 2048-sample frame into a 1024-point complex transform (x[2n] + i x[2n+1]) and
// pay a w2048 twist on each side.  A 1024-sample frame would fill only half of that transform.  Here frames f and f + 1 of an
// utterance ride together as z[n] = a[n] + i b[n]: lane l, slot q holds sample n = l + 64 q of BOTH frames, the unchanged wave
// transform (fft_wave.h) gives Z, and fw_pair_split turns (Z[k], Z[N-k]) into the two Hermitian spectra A[k], B[k].  Z[N-k] sits
// in lane 64 - lane, slot 15 - r: the very place the 2048 kernels find their partner.  There is no twist and no w2048 table.
//
//   gl_iter_pair_kernel      one 64-lane workgroup per frame PAIR: load -> FFT -> split -> project both spectra on their magnitude
//     (+ _mom_)              rows -> merge (Z' = XA + i XB) -> inverse FFT -> window -> the two frames' win samples.  The lane that
//                            owns N - k computes the bitwise conjugates of this lane's XA[k], XB[k] from the same two numbers, so Z'
//                            is Hermitian-consistent without a second exchange; DC and Nyquist come out real by construction.
//   istft_frames_pair_kernel / stft_phase_pair_kernel   first pass and the X_best debug path: the 256-thread LDS transform, fed a pair.
//   analysis_pair_kernel     the pair form of analysis_wave_kernel: two magnitude rows of 513 floats share the exchange buffer.
//   (ola_kernel serves both sizes: it reads n_fft from the geometry.)
//
// Edges.  Pair p of an utterance is frames 2p, 2p + 1 of THAT utterance (items are B * ceil(F / 2)): a pair never spans two
// utterances.  When F is odd the last pair has one frame: its b half is loaded as zeros, its magnitude row is never read (the
// projection multiplies by 0 instead) and nothing of it is stored, so frame F -- the next utterance's first, or past the buffer --
// is neither read nor written.  The analysis kernel applies the same rule per utterance: frame f + 1 >= n_frames beside a live
// frame f gets the zero rows, f + 1 >= Fpad gets nothing.
// Cross-talk.  The two frames share one fp32 transform, so a frame's rounding error is relative to the LOUDER of the two.  That is
// invisible to Griffin-Lim (neighbouring frames overlap by 3/4 and have like levels) and stays below the analysis normalisation floor
// of 1e-5 at ordinary levels; the measured figure for a 40 dB step is in DESIGN section 8.
// As before: bitwise reproducible, independent of the rest of the batch, no atomics, no waits between workgroups.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "analysis_kernels.h"

namespace dctts {

constexpr int PAIR_N = 1024;          // n_fft = the complex transform length
constexpr int PAIR_BINS = 513;
constexpr int PAIR_ROW = 516;         // float offset of the second magnitude row in the exchange buffer (16-byte aligned)

template <bool MOM>
__device__ __forceinline__ void gl_iter_pair_body(const VocGeom& g, const float* __restrict__ y, const float* __restrict__ spec,
                                                  float* __restrict__ fr_out, int n_items, int per_xcd,
                                                  const float* __restrict__ y_prev = nullptr, float beta = 0.f) {
  __shared__ float2 ex[FW_EX];
  const int lane = threadIdx.x;
  const int item = (int)(blockIdx.x & 7) * per_xcd + (int)(blockIdx.x >> 3);
  if ((int)(blockIdx.x >> 3) >= per_xcd || item >= n_items) return;
  const int P = (g.F + 1) >> 1;                              // pairs per utterance
  const int b = item / P, f = 2 * (item - b * P);
  const bool two = f + 1 < g.F;                              // uniform: false for the last pair of an odd F
  const float* yb = y + (long)b * g.L;
  const float* ypb = MOM ? y_prev + (long)b * g.L : nullptr;
  const int n0 = f * g.hop - PAIR_N / 2;                     // signal index of frame f's sample 0 (librosa.stft, center=True)
  const int q_lo = g.lpad >> 6, q_hi = (g.lpad + g.win - 1) >> 6;      // lane-strided slots 64 q .. 64 q + 63 that touch the window
  auto sig = [&](int n) -> float {                           // np.pad(mode="reflect"); L > n_fft / 2 keeps both frames' indices inside [0, L)
    if (n < 0) n = -n; else if (n >= g.L) n = 2 * (g.L - 1) - n;
    return MOM ? fmaf(-beta, ypb[(unsigned)n], yb[(unsigned)n]) : yb[(unsigned)n];
  };
  float2 v[16];
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    v[q] = make_float2(0.f, 0.f);
    if (q >= q_lo && q <= q_hi) {                            // uniform
      const int i = lane + 64 * q;
      if (i >= g.lpad && i < g.lpad + g.win) {
        const float w = g.window[(unsigned)i];
        v[q].x = sig(n0 + i) * w;
        if (two) v[q].y = sig(n0 + g.hop + i) * w;
      }
    }
  }
  fw_passA_store<false>(v, ex, lane); __syncthreads();
  fw_passB_load<false>(v, ex, lane, g.w1024); __syncthreads();
  fw_passB_store(v, ex, lane); __syncthreads();
  fw_passC_load<false>(v, ex, lane, g.w1024); __syncthreads();          // v[r] = Z[lane + 64 r]
#pragma unroll
  for (int r = 0; r < 16; ++r) ex[fw_base(lane) + 68 * r] = v[r];
  if (lane == 0) ex[FW_N + FW_N / 16] = v[0];               // Z[N] = Z[0], where lane 0's "partner lane 64" formula looks for it
  __syncthreads();
  const float2* exp_ = ex + fw_base(64 - lane);              // Z[N - k], k = lane + 64 r, sits at fw_base(64 - lane) + 68 (15 - r)
  const float* spA = spec + ((long)b * g.F + f) * PAIR_BINS;
  const float* spB = two ? spA + PAIR_BINS : spA;            // (never read when the pair has one frame)
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int k = lane + 64 * r;
    const unsigned kk = (unsigned)min(k, PAIR_N - k);        // the magnitude rows hold k <= N / 2
    float2 A, Bv;
    fw_pair_split(v[r], exp_[68 * (15 - r)], A, Bv);
    // spec / max(1e-8, |est|) as spec * min(rsq(|est|^2), 1e8), as gl_iter_wave_kernel
    const float sa = spA[kk] * fminf(__builtin_amdgcn_rsqf(fmaf(A.x, A.x, A.y * A.y)), 1e8f);
    const float sb = (two ? spB[kk] : 0.f) * fminf(__builtin_amdgcn_rsqf(fmaf(Bv.x, Bv.x, Bv.y * Bv.y)), 1e8f);
    v[r] = fw_pair_merge(make_float2(sa * A.x, sa * A.y), make_float2(sb * Bv.x, sb * Bv.y));
  }
  __syncthreads();
  fw_passA_store<true>(v, ex, lane); __syncthreads();
  fw_passB_load<true>(v, ex, lane, g.w1024i); __syncthreads();
  fw_passB_store(v, ex, lane); __syncthreads();
  fw_passC_load<true>(v, ex, lane, g.w1024i);               // v[r] = N (a'[n] + i b'[n]), n = lane + 64 r
  float* outA = fr_out + ((long)b * g.F + f) * g.frs;
  float* outB = outA + g.frs;
  const float inv = 1.0f / (float)PAIR_N;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int n = lane + 64 * r, i = n - g.lpad;
    if (i >= 0 && i < g.win) {
      const float w = g.window[(unsigned)n];
      outA[(unsigned)i] = (v[r].x * inv) * w;
      if (two) outB[(unsigned)i] = (v[r].y * inv) * w;
    }
  }
}
// Register budget, from the compiler's resource report: the plain form takes 136 VGPRs and no scratch under the 3-waves budget; held to
// 128 (4 waves / SIMD) it spills 16 bytes a lane, so it is built for 3.  The momentum form fits 128 VGPRs without scratch and is built for 4.
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(3, 3)))
gl_iter_pair_kernel(const VocGeom g, const float* __restrict__ y, const float* __restrict__ spec, float* __restrict__ fr_out,
                    int n_items, int per_xcd) { gl_iter_pair_body<false>(g, y, spec, fr_out, n_items, per_xcd); }
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4, 4)))
gl_iter_pair_mom_kernel(const VocGeom g, const float* __restrict__ y, const float* __restrict__ y_prev, float beta,
                        const float* __restrict__ spec, float* __restrict__ fr_out, int n_items, int per_xcd) {
  gl_iter_pair_body<true>(g, y, spec, fr_out, n_items, per_xcd, y_prev, beta);
}

// grid (ceil(F / 2), B).  X: (B, F, 513) complex, or nullptr with spec (B, F, 513) real (first iteration: zero phase).
__global__ void __launch_bounds__(VOC_THREADS) istft_frames_pair_kernel(const VocGeom g, const float2* __restrict__ X,
                                                                        const float* __restrict__ spec, float* __restrict__ fr) {
  __shared__ float2 s[2][VOC_M];
  const int tid = threadIdx.x, f = 2 * blockIdx.x, b = blockIdx.y;
  const bool two = f + 1 < g.F;
  const long rowA = ((long)b * g.F + f) * PAIR_BINS;
  auto ldx = [&](long row, int kk) -> float2 {
    float2 v = X ? X[row + kk] : make_float2(spec[row + kk], 0.f);
    if (kk == 0 || kk == PAIR_N / 2) v.y = 0.f;            // irfft ignores the imaginary part of DC / Nyquist
    return v;
  };
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int k = tid + r * VOC_THREADS, kk = min(k, PAIR_N - k);
    float2 xa = ldx(rowA, kk), xb = two ? ldx(rowA + PAIR_BINS, kk) : make_float2(0.f, 0.f);
    if (k > PAIR_N / 2) { xa.y = -xa.y; xb.y = -xb.y; }      // the Hermitian half
    s[0][k] = fw_pair_merge(xa, xb);
  }
  __syncthreads();
  fft1024<true>(s, g.w1024, tid);
  float* outA = fr + ((long)b * g.F + f) * g.frs;
  float* outB = outA + g.frs;
  const float inv = 1.0f / (float)PAIR_N;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int n = tid + r * VOC_THREADS, i = n - g.lpad;
    if (i >= 0 && i < g.win) {
      const float2 z = s[1][n];
      outA[i] = (z.x * inv) * g.window[n];
      if (two) outB[i] = (z.y * inv) * g.window[n];
    }
  }
}

// grid (ceil(F / 2), B).  Xout = spec * est / max(1e-8, |est|), est = stft(istft(X_prev)) evaluated from the stored frames.
__global__ void __launch_bounds__(VOC_THREADS) stft_phase_pair_kernel(const VocGeom g, const float* __restrict__ fr,
                                                                      const float* __restrict__ spec, float2* __restrict__ Xout) {
  __shared__ float2 s[2][VOC_M];
  const int tid = threadIdx.x, f = 2 * blockIdx.x, b = blockIdx.y;
  const bool two = f + 1 < g.F;
  const float* fr_b = fr + (long)b * g.F * g.frs;
  auto sample = [&](int ff, int i) -> float {              // windowed input sample i of frame ff (librosa.stft, center=True)
    if (i < g.lpad || i >= g.lpad + g.win) return 0.f;
    int n = ff * g.hop + i - PAIR_N / 2;
    if (n < 0) n = -n; else if (n >= g.L) n = 2 * (g.L - 1) - n;
    return ola_sample(g, fr_b, n + PAIR_N / 2) * g.window[i];
  };
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int n = tid + r * VOC_THREADS;
    s[0][n] = make_float2(sample(f, n), two ? sample(f + 1, n) : 0.f);
  }
  __syncthreads();
  fft1024<false>(s, g.w1024, tid);
  const long rowA = ((long)b * g.F + f) * PAIR_BINS;
  for (int k = tid; k <= PAIR_N / 2; k += VOC_THREADS) {
    float2 est[2];
    fw_pair_split(s[1][k], s[1][(PAIR_N - k) & (PAIR_N - 1)], est[0], est[1]);
    for (int h = 0; h < (two ? 2 : 1); ++h) {
      const float mag = fmaxf(1e-8f, hypotf(est[h].x, est[h].y));
      const float sp = spec[rowA + h * PAIR_BINS + k];
      Xout[rowA + h * PAIR_BINS + k] = make_float2(sp * (est[h].x / mag), sp * (est[h].y / mag));
    }
  }
}

// analysis_wave_kernel's banded mel projection of one magnitude row staged in LDS: a quarter-wave (one DPP row of 16 lanes) sums one band in a
// fixed order, four bands per round.
__device__ __forceinline__ void an_mel_row(const AnGeom& g, const float* smag, float* __restrict__ mel_row, int lane, float inv_db) {
  const int qd = lane >> 4, j = lane & 15;
  for (int m0 = 0; m0 < g.n_mels; m0 += 4) {
    const int4* bp = g.bands + m0;
    const int4 b0 = bp[0], b1 = bp[1], b2 = bp[2], b3 = bp[3];
    const int4 bd = qd == 0 ? b0 : qd == 1 ? b1 : qd == 2 ? b2 : b3;       // lo, width (<= AN_BAND_MAX), offset, zero weight
    float acc = 0.f;
#pragma unroll
    for (int t = 0; t < AN_BAND_ROUNDS; ++t) {                 // past the band's width: the table's zero weight times bin 0
      const int i = j + 16 * t;
      const bool in = i < bd.y;
      acc = fmaf(g.bandw[(unsigned)(in ? bd.z + i : bd.w)], smag[in ? bd.x + i : 0], acc);
    }
    acc = an_dpp_add<0xB1>(acc); acc = an_dpp_add<0x4E>(acc); acc = an_dpp_add<0x141>(acc); acc = an_dpp_add<0x140>(acc);
    if (j == 0) mel_row[m0 + qd] = an_norm(acc, g.max_db, inv_db, g.ref_db);
  }
}

// y'[n] of the trimmed clip yb[0 .. Lt), n reflected against its ends (np.pad(mode="reflect")) and clamped so that a sample under a zero of the window
// table still reads inside the clip; y'[0] = y[0] through the coefficient, not a branch
__device__ __forceinline__ float an_pair_sig(const float* __restrict__ yb, int n, int Lt, float preemph) {
  if (n < 0) n = -n; else if (n >= Lt) n = 2 * (Lt - 1) - n;
  n = min(max(n, 0), Lt - 1);
  return an_preemph(yb[(unsigned)n], yb[(unsigned)max(n - 1, 0)], n > 0 ? preemph : 0.f);
}

// One frame PAIR per wave; items are B * ceil(Fpad / 2), dealt to the XCDs in contiguous runs.  ws (B, 3): start, end, n_frames of each utterance.
// mag (B, Fpad, 513) or null; mel (B, Fpad / r, n_mels) or null: either frame of a pair may be a multiple of r.  All 16 slots are loaded without a
// branch per sample (the window table is 0 outside the window, indices are clamped into the clip), so a lane's loads are all in flight at once.
AN_KERNEL void __launch_bounds__(64) analysis_pair_kernel(const AnGeom g, const float* __restrict__ wav, const int* __restrict__ ws,
                                                           float* __restrict__ mag, float* __restrict__ mel, int n_items, int per_xcd) {
  __shared__ float2 ex[FW_EX];
  const int lane = threadIdx.x;
  const int item = (int)(blockIdx.x & 7) * per_xcd + (int)(blockIdx.x >> 3);
  if ((int)(blockIdx.x >> 3) >= per_xcd || item >= n_items) return;
  const int P = (g.Fpad + 1) >> 1;
  const int b = item / P, f = 2 * (item - b * P);
  const int s = ws[3 * b], Lt = ws[3 * b + 1] - s, Fb = ws[3 * b + 2];
  const float inv_db = 1.0f / g.max_db;
  const float* yb = wav + (long)b * g.Lmax + s;
  float* mag_row[2]; float* mel_row[2]; bool live[2];          // all uniform
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int fh = f + h;
    const bool has = fh < g.Fpad;                                // frame Fpad of an odd Fpad is the next utterance's row 0: not ours
    live[h] = fh < Fb;
    mag_row[h] = has && mag ? mag + ((long)b * g.Fpad + fh) * PAIR_BINS : nullptr;
    mel_row[h] = has && mel && fh % g.r == 0 ? mel + ((long)b * (g.Fpad / g.r) + fh / g.r) * g.n_mels : nullptr;
    if (!live[h]) {                                              // reduce_frames' zero rows, and every row of an utterance without frames
      if (mag_row[h]) for (int k = lane; k < PAIR_BINS; k += 64) mag_row[h][k] = 0.f;
      if (mel_row[h]) for (int m = lane; m < g.n_mels; m += 64) mel_row[h][m] = 0.f;
      mag_row[h] = nullptr; mel_row[h] = nullptr;
    }
  }
  if (!live[0] || (!mag_row[0] && !mel_row[0] && !mag_row[1] && !mel_row[1])) return;
  // ---- load: y'[n] = y[s + n] - a y[s + n - 1] (y'[0] = y[s]), reflected against [0, Lt), times the window; the b half stays 0 when frame f + 1 is not live
  const int n0 = f * g.hop - PAIR_N / 2;
  float2 v[16];
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int i = lane + 64 * q;
    const float w = g.window[(unsigned)i];
    v[q] = fw_f2(an_pair_sig(yb, n0 + i, Lt, g.preemph) * w, live[1] ? an_pair_sig(yb, n0 + g.hop + i, Lt, g.preemph) * w : 0.f);
  }
  fw_passA_store<false>(v, ex, lane); an_sync();
  fw_passB_load<false>(v, ex, lane, g.w1024); an_sync();
  fw_passB_store(v, ex, lane); an_sync();
  fw_passC_load<false>(v, ex, lane, g.w1024); an_sync();          // v[r] = Z[lane + 64 r]
  // ---- one exchange: the lane that owns k = lane + 64 r (r < 8) needs Z[N - k], which lane 64 - lane holds in slot 15 - r (>= 8)
#pragma unroll
  for (int r = 8; r < 16; ++r) ex[fw_base(lane) + 68 * r] = v[r];
  if (lane == 0) ex[FW_N + FW_N / 16] = v[0];
  an_sync();
  const float2* exp_ = ex + fw_base(64 - lane);
  float mA[8], mB[8];
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    float2 A, Bv;
    fw_pair_split(v[r], exp_[68 * (15 - r)], A, Bv);
    mA[r] = __builtin_amdgcn_sqrtf(fmaf(A.x, A.x, A.y * A.y));
    mB[r] = __builtin_amdgcn_sqrtf(fmaf(Bv.x, Bv.x, Bv.y * Bv.y));
  }
  an_sync();                                                      // every lane has read its partners: the buffer is free
  float* smag = reinterpret_cast<float*>(ex);                     // two rows of 513 linear magnitudes, PAIR_ROW apart
#pragma unroll
  for (int r = 0; r < 8; ++r) { smag[lane + 64 * r] = mA[r]; smag[PAIR_ROW + lane + 64 * r] = mB[r]; }
  if (lane == 0) {                                                // Z[512] is its own partner: A[512] = Re, B[512] = Im
    smag[PAIR_N / 2] = __builtin_fabsf(v[8].x); smag[PAIR_ROW + PAIR_N / 2] = __builtin_fabsf(v[8].y);
  }
  an_sync();
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const float* sm = smag + h * PAIR_ROW;
    if (mag_row[h]) {
#pragma unroll
      for (int j = 0; j < 8; ++j) mag_row[h][(unsigned)(lane + 64 * j)] = an_norm(sm[lane + 64 * j], g.max_db, inv_db, g.ref_db);
      if (lane == 0) mag_row[h][PAIR_N / 2] = an_norm(sm[PAIR_N / 2], g.max_db, inv_db, g.ref_db);
    }
    if (mel_row[h]) an_mel_row(g, sm, mel_row[h], lane, inv_db);
  }
}

}  // namespace dctts
