// analysis_kernels.h -- the analysis direction of the reference's utils.py (get_spectrograms, utils.py:18-65, and the frame
// reduction of load_spectrograms, :155-164) as HIP kernels for gfx950: a RAGGED batch of waveforms -> normalised mel / linear
// magnitude targets.  Everything an utterance's length decides (trim bounds, frame count) stays on the device.
//   frame_power_ragged_kernel / trim_bounds_ragged_kernel   librosa.effects.trim per utterance length -> bounds, n_frames
//   full_bounds_kernel        trim = 0: bounds = (0, len), n_frames
//   analysis_wave_kernel      ONE WAVE PER FRAME (fft_wave.h, as gl_iter_wave_kernel): trim offset + pre-emphasis + reflect
//                             padding + window fused into the load -> 2048-point real FFT -> |S| staged in LDS -> the
//                             normalised dB row (mag) and, for every r-th frame, the banded mel projection (mel).
// No atomics, no inter-workgroup waits; every loop is bounded by a launch argument or a constant.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vocoder_kernels.h"

namespace dctts {

// Scalar fp32 arithmetic only in these kernels: the packed fp32 forms (two lanes of a register pair per instruction) are kept out of new code.
#ifdef __HIP_DEVICE_COMPILE__
#define AN_KERNEL __global__ __attribute__((target("no-packed-fp32-ops")))
#else
#define AN_KERNEL __global__
#endif

// __syncthreads(), spelled out: with target features of their own these kernels cannot inline the HIP header's plain inline functions (nor make_float2: fw_f2)
__device__ __forceinline__ void an_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

constexpr int AN_BAND_ROUNDS = 6;                       // a band is summed by 16 lanes in <= 6 rounds
constexpr int AN_BAND_MAX = 16 * AN_BAND_ROUNDS;        // widest mel band the gather accepts (the 22 050 Hz / 2048 / 80 basis: 7..83)

struct AnGeom {
  int Lmax, Fpad, r, n_mels;
  int hop;
  float preemph, max_db, ref_db;
  const float* window;       // (n_fft) padded periodic Hann
  const float2* w1024;
  const float2* w2048;
  const int4* bands;         // (n_mels) lo, width, offset into bandw, index of bandw's trailing 0
  const float* bandw;        // compact mel weights, band after band, then one 0
};

// n_frames of an utterance whose (trimmed) signal is [s, e): -1 where reflect padding is undefined, 0 for nothing left
// (half = n_fft / 2 of the handle)
__device__ __forceinline__ int an_frame_count(int len, int s, int e, int hop, int half) {
  if (len <= half) return -1;
  if (e <= s) return 0;
  return e - s <= half ? -1 : 1 + (e - s) / hop;
}
__device__ __forceinline__ void an_put_bounds(int b, int s, int e, int nf, int* __restrict__ ws, int* __restrict__ bounds,
                                              int* __restrict__ n_frames) {
  ws[3 * b] = s; ws[3 * b + 1] = e; ws[3 * b + 2] = nf;
  if (bounds) { bounds[2 * b] = s; bounds[2 * b + 1] = e; }
  if (n_frames) n_frames[b] = nf;
}
__device__ __forceinline__ int an_len(const int* __restrict__ lengths, int b, int Lmax) { return min(max(lengths[b], 0), Lmax); }

// trim = 0.  grid (ceil(B / 64)), block 64.
AN_KERNEL void __launch_bounds__(64) full_bounds_kernel(const int* __restrict__ lengths, int B, int Lmax, int hop, int half, int* __restrict__ ws,
                                                         int* __restrict__ bounds, int* __restrict__ n_frames) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  const int len = an_len(lengths, b, Lmax);
  an_put_bounds(b, 0, len, an_frame_count(len, 0, len, hop, half), ws, bounds, n_frames);
}

// frame_power_kernel for a ragged batch: utterance b has lengths[b] samples of its Lmax-long row; frames past its own count, and an
// utterance too short to reflect-pad, are left alone (trim_bounds_ragged_kernel does not read them).  grid (1 + Lmax / fhop, B).
AN_KERNEL void __launch_bounds__(256) frame_power_ragged_kernel(const float* __restrict__ y, const int* __restrict__ lengths,
                                                                 float* __restrict__ pw, int Lmax, int n_tf, int flen, int fhop) {
  __shared__ float red[256];
  const int tid = threadIdx.x, j = blockIdx.x, b = blockIdx.y;
  const int L = an_len(lengths, b, Lmax);
  if (L <= flen / 2 || j > L / fhop) return;                 // uniform
  const float* yb = y + (long)b * Lmax;
  float acc = 0.f;
  for (int i = tid; i < flen; i += 256) {
    int n = j * fhop + i - flen / 2;
    if (n < 0) n = -n; else if (n >= L) n = 2 * (L - 1) - n;
    const float v = yb[n];
    acc += v * v;
  }
  red[tid] = acc;
  an_sync();
  for (int o = 128; o > 0; o >>= 1) { if (tid < o) red[tid] += red[tid + o]; an_sync(); }
  if (tid == 0) pw[(long)b * n_tf + j] = red[0] / (float)flen;
}

// trim_bounds_kernel for a ragged batch, plus the frame count the analysis kernel needs.  A clip whose loudest frame has no power at all
// keeps nothing (n_frames 0).  grid (B), block 256.
AN_KERNEL void __launch_bounds__(256) trim_bounds_ragged_kernel(const float* __restrict__ pw, const int* __restrict__ lengths,
                                                                 int Lmax, int n_tf, int flen, int fhop, float top_db, int hop, int half,
                                                                 int* __restrict__ ws, int* __restrict__ bounds, int* __restrict__ n_frames) {
  __shared__ float smax[256];
  __shared__ int sfirst[256], slast[256];
  const int tid = threadIdx.x, b = blockIdx.x;
  const int L = an_len(lengths, b, Lmax);
  if (L <= flen / 2 || L <= half) {                  // uniform
    if (tid == 0) an_put_bounds(b, 0, L, -1, ws, bounds, n_frames);
    return;
  }
  const int nt = 1 + L / fhop;
  const float* p = pw + (long)b * n_tf;
  float mx = 0.f;
  for (int j = tid; j < nt; j += 256) mx = fmaxf(mx, p[j]);
  smax[tid] = mx;
  an_sync();
  for (int o = 128; o > 0; o >>= 1) { if (tid < o) smax[tid] = fmaxf(smax[tid], smax[tid + o]); an_sync(); }
  const float pmax = smax[0];
  const float ref = 10.0f * log10f(fmaxf(1e-10f, pmax));
  int first = 0x7fffffff, last = -1;
  for (int j = tid; j < nt; j += 256) {
    const float db = 10.0f * log10f(fmaxf(1e-10f, p[j])) - ref;
    if (db > -top_db && pmax > 0.f) { if (j < first) first = j; if (j > last) last = j; }
  }
  sfirst[tid] = first; slast[tid] = last;
  an_sync();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) { sfirst[tid] = min(sfirst[tid], sfirst[tid + o]); slast[tid] = max(slast[tid], slast[tid + o]); }
    an_sync();
  }
  if (tid == 0) {
    int s = 0, e = 0;
    if (slast[0] >= 0) { s = sfirst[0] * fhop; e = (slast[0] + 1) * fhop; if (e > L) e = L; }
    an_put_bounds(b, s, e, an_frame_count(L, s, e, hop, half), ws, bounds, n_frames);
  }
}

template <int CTRL>
__device__ __forceinline__ float an_dpp_add(float v) {
  return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, true));
}

// clip((20 log10(max(1e-5, x)) - ref_db + max_db) / max_db, 1e-8, 1) (utils.py:56-61); v_log_f32 is ~1 ulp of log2 x.  The division is one
// Newton step on t * (1 / max_db) (inv_db is the rounded reciprocal): three instructions instead of the ~10 of an IEEE divide, the same quotient up to its last bit.
__device__ __forceinline__ float an_norm(float x, float max_db, float inv_db, float ref_db) {
  const float t = 6.02059991327962390f * __builtin_amdgcn_logf(fmaxf(1e-5f, x)) - ref_db + max_db;          // 20 log10(2) * log2(x)
  float q = t * inv_db;
  q = fmaf(fmaf(-q, max_db, t), inv_db, q);
  return fminf(fmaxf(q, 1e-8f), 1.f);
}

// yn - a yp with two roundings, as numpy's float32 expression in audio.spectrograms_of (no contraction into one fma)
__device__ __forceinline__ float an_preemph(float yn, float yp, float a) {
#pragma clang fp contract(off)
  const float p = a * yp;
  return yn - p;
}

// One frame per wave.  ws (B, 3): start, end, n_frames of each utterance.  mag (B, Fpad, 1025) or null; mel (B, Fpad / r, n_mels) or null.
// Workgroup w runs on XCD w % 8: items are dealt out so that each XCD gets a contiguous run of frames (gl_iter_wave_kernel's rule).
// QLO..QHI: the lane-strided slots (128 q .. 128 q + 127) that are loaded; the window must lie inside them.  Compile-time, so that no uniform branch sits
// between the slots and a lane's ~50 loads are all in flight at once: <3, 12> for the reference's 1102-sample window, <0, 15> for any other.
template <int QLO, int QHI>
AN_KERNEL void __launch_bounds__(64) analysis_wave_kernel(const AnGeom g, const float* __restrict__ wav, const int* __restrict__ ws,
                                                           float* __restrict__ mag, float* __restrict__ mel, int n_items, int per_xcd) {
  __shared__ float2 ex[FW_EX];
  const int lane = threadIdx.x;
  const int item = (int)(blockIdx.x & 7) * per_xcd + (int)(blockIdx.x >> 3);
  if ((int)(blockIdx.x >> 3) >= per_xcd || item >= n_items) return;
  const int b = item / g.Fpad, f = item - b * g.Fpad;
  const bool want_mel = mel != nullptr && f % g.r == 0;          // uniform
  if (!mag && !want_mel) return;
  float* mag_row = mag ? mag + ((long)b * g.Fpad + f) * VOC_BINS : nullptr;
  float* mel_row = want_mel ? mel + ((long)b * (g.Fpad / g.r) + f / g.r) * g.n_mels : nullptr;
  const float inv_db = 1.0f / g.max_db;
  const int s = ws[3 * b], Lt = ws[3 * b + 1] - s, Fb = ws[3 * b + 2];
  if (f >= Fb) {                                                 // reduce_frames' zero rows, and every row of an utterance without frames
    if (mag_row) for (int k = lane; k < VOC_BINS; k += 64) mag_row[k] = 0.f;
    if (mel_row) for (int m = lane; m < g.n_mels; m += 64) mel_row[m] = 0.f;
    return;
  }
  // ---- load: y'[n] = y[s + n] - a y[s + n - 1] (y'[0] = y[s]), reflected against [0, Lt), times the window.  No branch per sample: a slot's samples
  // outside the window have weight 0 and read a clamped (in-range) index, so all the loads of a lane can be in flight together.
  const float* yb = wav + (long)b * g.Lmax + s;
  const int n0 = f * g.hop - VOC_NFFT / 2;
  float2 v[16];
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    v[q] = fw_f2(0.f, 0.f);
    if (q >= QLO && q <= QHI) {
      const int i0 = 2 * (lane + 64 * q);
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int i = i0 + h;
        int n = n0 + i;
        if (n < 0) n = -n; else if (n >= Lt) n = 2 * (Lt - 1) - n;      // np.pad(mode="reflect"): 0 <= n < Lt under the window because Lt > n_fft / 2
        n = min(max(n, 0), Lt - 1);
        const float yn = yb[(unsigned)n], yp = yb[(unsigned)max(n - 1, 0)];
        const float x = an_preemph(yn, yp, n > 0 ? g.preemph : 0.f) * g.window[(unsigned)i];      // (n = 0: y'[0] = y[s], through the coefficient, not a branch)
        if (h == 0) v[q].x = x; else v[q].y = x;
      }
    }
  }
  // ---- 1024-point complex FFT of z[n] = x[2n] + i x[2n+1]
  fw_passA_store<false>(v, ex, lane); an_sync();
  fw_passB_load<false>(v, ex, lane, g.w1024); an_sync();
  fw_passB_store(v, ex, lane); an_sync();
  fw_passC_load<false>(v, ex, lane, g.w1024); an_sync();          // v[r] = Z[lane + 64 r]
  // ---- one exchange: the lane that owns k = lane + 64 r (r < 8) needs Z[M - k], which lane 64 - lane holds in slot 15 - r (>= 8)
#pragma unroll
  for (int r = 8; r < 16; ++r) ex[fw_base(lane) + 68 * r] = v[r];
  if (lane == 0) ex[FW_N + FW_N / 16] = v[0];                    // Z[M] = Z[0], where lane 0's "partner lane 64" formula looks for it
  an_sync();
  const float2* exp_ = ex + fw_base(64 - lane);
  float m1[8], m2[8];
  // ---- post-twist from the pair (Z[k], Z[M-k]): S[k] = E + Dw/i, S[M-k] = conj(E) + conj(Dw)/i, E = (a + conj c)/2, Dw = W^k (a - conj c)/2
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const int k = lane + 64 * r;
    const float2 a = v[r], c = exp_[68 * (15 - r)];
    const float2 w = g.w2048[(unsigned)k];
    const float2 E = fw_f2(0.5f * (a.x + c.x), 0.5f * (a.y - c.y));
    const float2 D = fw_f2(0.5f * (a.x - c.x), 0.5f * (a.y + c.y));
    const float2 Dw = fw_mul(D, w);
    const float2 e1 = fw_f2(E.x + Dw.y, E.y - Dw.x);       // S[k]
    const float2 e2 = fw_f2(E.x - Dw.y, E.y + Dw.x);       // conj-sign of S[M-k]'s imaginary part: only |.| is used
    m1[r] = __builtin_amdgcn_sqrtf(fmaf(e1.x, e1.x, e1.y * e1.y));
    m2[r] = __builtin_amdgcn_sqrtf(fmaf(e2.x, e2.x, e2.y * e2.y));
  }
  an_sync();                                               // every lane has read its partners: the buffer is free
  float* smag = reinterpret_cast<float*>(ex);                    // 1025 linear magnitudes
#pragma unroll
  for (int r = 0; r < 8; ++r) { smag[lane + 64 * r] = m1[r]; smag[VOC_M - lane - 64 * r] = m2[r]; }
  if (lane == 0) smag[VOC_M / 2] = __builtin_amdgcn_sqrtf(fmaf(v[8].x, v[8].x, v[8].y * v[8].y));      // S[512] = conj Z[512]
  an_sync();
  if (mag_row) {
#pragma unroll
    for (int j = 0; j < 16; ++j) mag_row[(unsigned)(lane + 64 * j)] = an_norm(smag[lane + 64 * j], g.max_db, inv_db, g.ref_db);
    if (lane == 0) mag_row[VOC_M] = an_norm(smag[VOC_M], g.max_db, inv_db, g.ref_db);
  }
  if (mel_row) {
    // ---- banded mel projection: a quarter-wave (one DPP row of 16 lanes) sums one band in a fixed order, four bands per round
    const int qd = lane >> 4, j = lane & 15;
    for (int m0 = 0; m0 < g.n_mels; m0 += 4) {
      const int4* bp = g.bands + m0;                             // uniform address: the four descriptors of the round, picked by quarter
      const int4 b0 = bp[0], b1 = bp[1], b2 = bp[2], b3 = bp[3];
      const int4 bd = qd == 0 ? b0 : qd == 1 ? b1 : qd == 2 ? b2 : b3;       // lo, width (<= AN_BAND_MAX), offset, zero weight
      float acc = 0.f;
#pragma unroll
      for (int t = 0; t < AN_BAND_ROUNDS; ++t) {                 // past the band's width: the table's zero weight times bin 0, so no load waits for a branch
        const int i = j + 16 * t;
        const bool in = i < bd.y;
        acc = fmaf(g.bandw[(unsigned)(in ? bd.z + i : bd.w)], smag[in ? bd.x + i : 0], acc);
      }
      acc = an_dpp_add<0xB1>(acc); acc = an_dpp_add<0x4E>(acc); acc = an_dpp_add<0x141>(acc); acc = an_dpp_add<0x140>(acc);
      if (j == 0) mel_row[m0 + qd] = an_norm(acc, g.max_db, inv_db, g.ref_db);
    }
  }
}

}  // namespace dctts
