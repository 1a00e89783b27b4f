// train_gemm3_kernel.h -- the training GEMM on the bf16 matrix pipe (opt-in: dctts_train_set_split_bf16_terms(t, 3)); DESIGN section 10.
//
// Same contract as gemm_kernel<TA, TB> (train_kernels.h): GemmParams, 128 x 128 output tile per workgroup, z = split-K slice / batch /
// batch x split, beta, nseg segments with (possibly negative) row offsets, zero fill outside M, N and [kbeg, kend).  The arithmetic is the
// three-term split of split_bf16.h: every fp32 element of BOTH operands is hi + mid + lo (three bf16, exact), and per 16 k six
// v_mfma_f32_32x32x16_bf16 products are accumulated in fp32, small terms first: lo.hi, hi.lo, mid.mid, mid.hi, hi.mid, hi.hi.
//
// Data movement (in training both operands change every step, so nothing is packed ahead of the launch):
//   * a stage is 16 k.  Per operand a thread fetches 8 floats (k-contiguous storage) or 16 floats (k-major storage, half of the workgroup per
//     operand) as float4, keeps them in registers across the contraction of the current stage, then splits them ONCE and stores three bf16
//     planes: the MFMA loop has no conversion in it, and an element is split once per workgroup, not once per wave.
//   * LDS plane = [half h of the 16 k][row slot][8 bf16 = 16 bytes]: the 8 consecutive k a lane feeds to one MFMA are one ds_read_b128.
//     slot(row, h) = row ^ (bit 4 of row) << 1 ^ 9 h, a permutation inside every group of 16 rows, so:
//       - MFMA read: lanes (l & 31 = row, l >> 5 = h); 16 consecutive lanes read 16 different slots of one aligned group of 16 = 256
//         contiguous bytes = every one of the 64 banks once;
//       - k-contiguous store (thread = (row = tid >> 1, h = tid & 1), one 16-byte write per plane): 16 consecutive lanes are 8 rows of one
//         aligned group of 8 in both halves; 9 h flips bit 3 of the slot, so the two halves land in the two 128-byte halves of a 256-byte window;
//       - k-major store (lane = (k quad kq = l & 3, 4 columns cg = l >> 2), for each of its 4 rows one 8-byte write per plane, the
//         transposition): in one instruction 32 lanes write rows 4 cg + i, cg = 0..7, for both halves and both 8-byte sides; bits (cg1, cg0)
//         pick slot bits (3, 2), cg2 = bit 4 of the row flips slot bit 1, h flips slot bit 0: 16 slots x 2 sides = all 64 banks once.
//     No padding is needed: 2 buffers x 2 operands x 3 planes x 4 KB = 48 KB, three workgroups per CU by LDS.
//   * per 16 k a wave (64 x 64 of the tile, 2 x 2 MFMA tiles) issues 12 ds_read_b128 for 24 MFMAs.
// inf in an operand gives NaN (inf - inf in the split) where gemm_kernel gives +-inf; |x| below ~2^-100 loses its low terms to bf16 underflow.
#pragma once
#include "split_bf16.h"
#include "train_kernels.h"

namespace dctts {

__device__ __forceinline__ int g3_slot(int row, int h) { return row ^ (((row >> 4) & 1) << 1) ^ (h * 9); }

// one operand's part of a stage: fetch (global -> registers) and store (registers -> split -> three LDS planes).
// KM: the stored matrix is k-major (rows of the stored matrix are k; a float4 runs along the operand's rows).  SIDE: which half of the
// workgroup moves a k-major operand (0: threads 0..127, 1: threads 128..255).
template <bool KM, int SIDE>
struct G3Mover {
  const int tid, r0, R, ld;            // r0: first row of the tile, R: rows of the operand (M or N)
  __device__ __forceinline__ bool active() const { return !KM || (tid >> 7) == SIDE; }
  __device__ __forceinline__ void fetch(const float* P, int k0, int kend, float4 (&v)[4]) const {
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (KM) {
      if (!active()) return;
      const int t = tid & 127, kq = t & 3, col = r0 + (((t >> 2) & 15) + 16 * (t >> 6)) * 4;
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        const int k = k0 + kq * 4 + f;
        v[f] = z4;
        if (k < kend && col < R) v[f] = *reinterpret_cast<const float4*>(P + (long)k * ld + col);
      }
    } else {
      const int row = r0 + (tid >> 1), kb = k0 + (tid & 1) * 8;
#pragma unroll
      for (int f = 0; f < 2; ++f) {
        v[f] = z4;
        if (row < R && kb + f * 4 < kend) v[f] = *reinterpret_cast<const float4*>(P + (long)row * ld + kb + f * 4);
      }
    }
  }
  // S: the operand's three planes of one buffer, 256 uint4 each
  __device__ __forceinline__ void store(uint4 (*S)[256], const float4 (&v)[4]) const {
    if constexpr (KM) {
      if (!active()) return;
      const int t = tid & 127, kq = t & 3, cg = ((t >> 2) & 15) + 16 * (t >> 6), h = kq >> 1;
      auto el = [](const float4& q, int i) { return i == 0 ? q.x : (i == 1 ? q.y : (i == 2 ? q.z : q.w)); };
#pragma unroll
      for (int i = 0; i < 4; ++i) {      // row cg * 4 + i of the tile: its 4 consecutive k
        uint2 hi, mid, lo;
        split_bf16_pair3(el(v[0], i), el(v[1], i), hi.x, mid.x, lo.x); split_bf16_pair3(el(v[2], i), el(v[3], i), hi.y, mid.y, lo.y);
        const int idx = (h * 128 + g3_slot(cg * 4 + i, h)) * 2 + (kq & 1);
        reinterpret_cast<uint2*>(S[0])[idx] = hi; reinterpret_cast<uint2*>(S[1])[idx] = mid; reinterpret_cast<uint2*>(S[2])[idx] = lo;
      }
    } else {
      const int row = tid >> 1, h = tid & 1;
      uint4 hi, mid, lo;
      split_bf16_pair3(v[0].x, v[0].y, hi.x, mid.x, lo.x); split_bf16_pair3(v[0].z, v[0].w, hi.y, mid.y, lo.y);
      split_bf16_pair3(v[1].x, v[1].y, hi.z, mid.z, lo.z); split_bf16_pair3(v[1].z, v[1].w, hi.w, mid.w, lo.w);
      const int idx = h * 128 + g3_slot(row, h);
      S[0][idx] = hi; S[1][idx] = mid; S[2][idx] = lo;
    }
  }
};

template <bool TA, bool TB>
__global__ void __launch_bounds__(256) gemm3_kernel(const GemmParams p) {
  constexpr int BM = 128, BN = 128, BK = 16;
  __shared__ uint4 Ss[2][2][3][256];                                     // [buffer][A, B][hi, mid, lo][half * 128 + slot]: 48 KB
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
  const int zb = p.batched ? (int)blockIdx.z / p.nsplit : 0, zk = p.batched ? (int)blockIdx.z % p.nsplit : (int)blockIdx.z;
  const int kbeg = zk * p.kchunk, kend = min(p.K, kbeg + p.kchunk);
  const float* pA = p.A + (long)zb * p.a_zs;
  const float* pB = p.B + (long)zb * p.b_zs;
  const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64, l31 = lane & 31, lhi = lane >> 5;
  const G3Mover<TA, 0> ma{tid, m0, p.M, p.lda};
  const G3Mover<!TB, 1> mb{tid, n0, p.N, p.ldb};
  tf32x16 acc[4];
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[q][j] = 0.f;
  float4 ra[4], rb[4];
  ma.fetch(pA, kbeg, kend, ra); mb.fetch(pB, kbeg, kend, rb);
  ma.store(Ss[0][0], ra); mb.store(Ss[0][1], rb);
  __syncthreads();
  // this lane's fragments: row l31 of each 32-row MFMA tile, k half lhi
  int ia[2], ib[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) { ia[i] = lhi * 128 + g3_slot(wm + i * 32 + l31, lhi); ib[i] = lhi * 128 + g3_slot(wn + i * 32 + l31, lhi); }
  int buf = 0, seg = 0;
  for (int k0 = kbeg; k0 < kend || seg + 1 < p.nseg; k0 += BK) {
    if (k0 >= kend) { k0 = kbeg; ++seg; }                               // the stage in LDS is the first one of the next segment
    bool more = k0 + BK < kend;
    int kn = k0 + BK;
    if (!more && seg + 1 < p.nseg) { more = true; kn = kbeg; pA += p.a_ss; pB += p.b_ss; }     // prefetch across the segment boundary
    if (more) { ma.fetch(pA, kn, kend, ra); mb.fetch(pB, kn, kend, rb); }                      // in flight while this stage is contracted
    bf16x8_t a[3][2], b[3][2];                                           // [hi, mid, lo][MFMA tile]
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        a[t][i] = __builtin_bit_cast(bf16x8_t, Ss[buf][0][t][ia[i]]);
        b[t][i] = __builtin_bit_cast(bf16x8_t, Ss[buf][1][t][ib[i]]);
      }
    // small products first; the four accumulators take turns, so two MFMAs on one accumulator are four instructions apart
    auto prod = [&](const bf16x8_t (&x)[2], const bf16x8_t (&y)[2]) {
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[q] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x[q >> 1], y[q & 1], acc[q], 0, 0, 0);
    };
    prod(a[2], b[0]); prod(a[0], b[2]); prod(a[1], b[1]);                // lo.hi, hi.lo, mid.mid
    prod(a[1], b[0]); prod(a[0], b[1]); prod(a[0], b[0]);                // mid.hi, hi.mid, hi.hi
    if (more) { ma.store(Ss[buf ^ 1][0], ra); mb.store(Ss[buf ^ 1][1], rb); }
    __syncthreads();
    buf ^= 1;
  }
  float* C = p.C + (long)blockIdx.z * p.c_zstride;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int col = n0 + wn + (q & 1) * 32 + l31;
    if (col >= p.N) continue;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int row = m0 + wm + (q >> 1) * 32 + (j & 3) + 8 * (j >> 2) + 4 * lhi;      // accumulator layout of v_mfma_f32_32x32x16_bf16 = that of 32x32x2_f32
      if (row < p.M) { float* c = C + (long)row * p.ldc + col; *c = (p.beta ? *c : 0.f) + acc[q][j]; }
    }
  }
}

}  // namespace dctts
