// Fused flash-style attention (fwd + bwd) for gfx950, head_dim = 64.
//
// Design (guide: cdna_hip_programming.md §B "Fused attention prefill"):
//  * swapped-operand QK^T — compute mfma(K, Q) so each lane owns ONE
//    query row (col = lane&31) and its softmax state (m, l) is
//    lane-local: the row reduce is a per-reg max/sum + one
//    __shfl_xor(32), no LDS round trip;
//  * v_mfma_f32_32x32x16_bf16 tiles; the PER-WAVE operands (Q/dO in fwd
//    and dq; K/V resident in dkv) load directly from global memory
//    (A/B fragment layout = 8 contiguous d-elements per lane = a
//    row-major [T, D] slice; strides passed in, so the fused-QKV views
//    are consumed with zero transpose copies).  The BLOCK-SHARED
//    operands (K in fwd; K/V in dq; Q/dO in dkv) are staged ONCE per
//    block into stride-72 LDS row images — bank-conflict-free for the
//    b128 fragment reads — instead of 4x-redundant per-wave global
//    loads (r2: fwd +40%, bwd +77%; PMC showed 60-70% WAIT_ANY before);
//  * P relayout for the PV mfma via v_cvt_pk_bf16_f32 + permlane32_swap
//    (guide T12): converts the 16 f32 score regs into the bf16 A/B
//    fragment in-register;
//  * O is accumulated TRANSPOSED (O^T[d][q], col = lane&31 = q) so the
//    online rescale multiplies lane-local registers;
//  * per block: 4 waves × 32 query rows; V^T (and in backward dO^T/Q^T/
//    K^T) tiles staged transposed in LDS (row stride 40 elems — bank-
//    conflict-free ds_read_b128);
//  * softmax in base-2 (v_exp_f32 is exp2): saved "lse" is
//    lse2 = m2 + log2(l); backward recomputes P = exp2(s*scale*log2e - lse2).
//
// Backward = 3 small kernels (delta, dq, dkv): dq re-derives dS with
// the fwd (lane-owns-q) orientation; dkv uses the mirrored
// (lane-owns-key) orientation so dK^T/dV^T accumulate lane-locally.
//
// One kernel body per pass.  The occupancy variants are template
// instantiations picked by the launchers from an environment knob:
//   attn_fwd_kernel<MINW, KLDS>      QN_ATTN_FWD_OCC (3 | 4), QN_ATTN_KLDS (1 | 0)
//   attn_bwd_dq_kernel<MINW, PIPE>   QN_ATTN_DQ_OCC  (3 | 2 pipelined, 4 not)
//   attn_bwd_dkv_kernel<MINW, PIPE>  QN_ATTN_DKV_OCC (2 pipelined, 3 not)
// All three run a 1-D grid of T/128 * B*H blocks; attn_block_of (attn.h)
// maps the block id to (row block, head), QN_ATTN_ORDER (balanced | linear)
// picks the order for causal launches.
// The passes share the leaf helpers below (row images, S/dP chain,
// transposed-tile MFMAs, scatter store, q-major causal window) and take
// their tensors as pointer + AttnView strides (attn.h).
// tests/test_attention_variants_gpu.py runs every instantiation.
//
// Replaces reference F.scaled_dot_product_attention
// (utils/GPT2/gpt2_attention.py:156).
#include <cstdlib>
#include <cstring>

#include "attn.h"
#include "common.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;

#define LOG2E 1.4426950408889634f
#define TPAD 40  // LDS transpose-tile row stride (elems): conflict-free

// ---- cvt_pk + permlane relayout (guide T12) --------------------------------
// 8 f32 regs (this lane's rows r..r+7 of a 32-col MFMA D tile) -> one
// bf16x8 fragment whose 8 elements are rows (lane>>5)*8..+7 at this
// lane's column: the A/B operand layout of mfma_f32_32x32x16_bf16.
__device__ __forceinline__ unsigned cvt_pk_bf16(float lo, float hi) {
  unsigned r;
  // s_nop 1 = the 2 VALU->v_permlane wait states (guide §5.5 T21 hazard;
  // hipcc pads nothing across an asm boundary for the following builtin)
  asm volatile("v_cvt_pk_bf16_f32 %0, %1, %2\n\ts_nop 1" : "=v"(r) : "v"(lo), "v"(hi));
  return r;
}

__device__ __forceinline__ bf16x8 relayout8(const float* p) {
  unsigned a0 = cvt_pk_bf16(p[0], p[1]);
  unsigned a1 = cvt_pk_bf16(p[2], p[3]);
  unsigned a2 = cvt_pk_bf16(p[4], p[5]);
  unsigned a3 = cvt_pk_bf16(p[6], p[7]);
  {
    auto r = __builtin_amdgcn_permlane32_swap(a0, a2, false, false);
    a0 = r[0]; a2 = r[1];
  }
  {
    auto r = __builtin_amdgcn_permlane32_swap(a1, a3, false, false);
    a1 = r[0]; a3 = r[1];
  }
  union { unsigned u[4]; bf16x8 v; } out;
  out.u[0] = a0; out.u[1] = a1; out.u[2] = a2; out.u[3] = a3;
  return out.v;
}

// load one 32x32x16 A/B fragment straight from a strided [T, 64] slice:
// lane row = base_row + (l&31), elems d0 + (l>>5)*8 .. +8 (bf16, 16B).
__device__ __forceinline__ bf16x8 frag_ld(const unsigned short* base,
                                          long long row_stride, int row0,
                                          int d0, int lane) {
  const unsigned short* p = base + (long long)(row0 + (lane & 31)) * row_stride +
                            d0 + ((lane >> 5) << 3);
  return *reinterpret_cast<const bf16x8*>(p);
}

// per-lane fragment base pointer: subsequent tiles advance it by
// 32*row_stride and the 4 kt-fragments sit at +16 elem immediates — the
// per-tile 64-bit address rebuild was a major VALU cost (cf. gemm.hip).
__device__ __forceinline__ const unsigned short* frag_base(
    const unsigned short* base, long long row_stride, int row0, int lane) {
  return base + (long long)(row0 + (lane & 31)) * row_stride + ((lane >> 5) << 3);
}

__device__ __forceinline__ bf16x8 frag_at(const unsigned short* p, int kt) {
  return *reinterpret_cast<const bf16x8*>(p + kt * 16);
}

__device__ __forceinline__ const unsigned short* stage_base(
    const unsigned short* src, long long row_stride, int row0) {
  int r = threadIdx.x & 31;
  int d0 = (threadIdx.x >> 5) << 3;
  return src + (long long)(row0 + r) * row_stride + d0;
}

__device__ __forceinline__ s16x8 stage_at(const unsigned short* p) {
  return *reinterpret_cast<const s16x8*>(p);
}

// MFMA D-tile row of register r for this lane (32x32 layout)
__device__ __forceinline__ int drow(int r, int lane) {
  return (r & 3) + ((r >> 2) << 3) + ((lane >> 5) << 2);
}

// cooperative transpose-stage of a [32, 64] strided tile into LDS
// t[64][TPAD] (t[d][r]); 256 threads, 8 contiguous elems each.  Split
// into load (stage_at: issue early, overlap with compute — T14) and write.
// thread -> (row, d-chunk) map r = t&31, d0 = (t>>5)*8: the ds_write_u16
// bank pattern is then 4-way (r spreads banks) instead of 16-way.
__device__ __forceinline__ void stage_wr(unsigned short* t, s16x8 v) {
  int r = threadIdx.x & 31;
  int d0 = (threadIdx.x >> 5) << 3;
#pragma unroll
  for (int j = 0; j < 8; ++j) t[(d0 + j) * TPAD + r] = (unsigned short)v[j];
}

// ---- row images: [32][KPAD] row-major LDS copies of a staged tile ---------
// The block-shared MFMA operands are read from these as b128 fragments;
// stride 72 keeps those reads bank-conflict-free.  Both offsets are
// loop-invariant: each kernel computes them once.
#define KPAD 72

// this thread's 8 staged elements (same row/d-chunk map as stage_wr)
__device__ __forceinline__ int rowimg_st_off() {
  return (threadIdx.x & 31) * KPAD + ((threadIdx.x >> 5) << 3);
}

// this lane's kt=0 A/B fragment; kt = 1..3 sit at +16 elems
__device__ __forceinline__ int rowimg_frag_off(int lane) {
  return (lane & 31) * KPAD + ((lane >> 5) << 3);
}

__device__ __forceinline__ void rowimg_st(unsigned short* img, int st_off, s16x8 v) {
  *reinterpret_cast<s16x8*>(img + st_off) = v;
}

// S and dP for one 32x32 tile: s = A·x, dp = B·y over D = 64, the two
// chains interleaved.  a/b point at this lane's fragment in two row
// images, x/y are the wave's register fragments: dq passes the K/V images
// with its Q/dO fragments, dkv the Q/dO images with its K/V fragments.
__device__ __forceinline__ void sdp_chain(
    const unsigned short* a, const unsigned short* b, const bf16x8 (&x)[4],
    const bf16x8 (&y)[4], const f32x16& zc, f32x16& s, f32x16& dp) {
  s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_at(a, 0), x[0], zc, 0, 0, 0);
  dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_at(b, 0), y[0], zc, 0, 0, 0);
#pragma unroll
  for (int t = 1; t < 4; ++t) {
    s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_at(a, t), x[t], s, 0, 0, 0);
    dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_at(b, t), y[t], dp, 0, 0, 0);
  }
}

// acc^T[mt*32 + .][col] += t[mt*32 + .][0..32) · (b0 | b1): the A operand
// is rows mt*32.. of a transposed tile t[64][TPAD], b0/b1 the relayouted
// fragments of the tile's two 16-row halves.  One accumulator by
// reference per call — an accumulator ARRAY passed by pointer spills.
__device__ __forceinline__ void tmfma2(const unsigned short* t, int mt, int lane,
                                       bf16x8 b0, bf16x8 b1, f32x16& acc) {
  const unsigned short* a = &t[(mt * 32 + (lane & 31)) * TPAD + ((lane >> 5) << 3)];
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_at(a, 0), b0, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_at(a, 1), b1, acc, 0, 0, 0);
}

// scatter-store half mt of a transposed accumulator (lane owns one output
// row, its registers are d = mt*32 + drow(r)) into that row as bf16
__device__ __forceinline__ void drow_st(unsigned short* row, int mt, int lane, f32x16 acc) {
#pragma unroll
  for (int r = 0; r < 16; ++r) row[mt * 32 + drow(r, lane)] = f32_to_bf16(acc[r]);
}

// ---- causal window, q-major loops (fwd, dq): block owns q rows
// [q0, q0+128), wave rows [qw, qw+32), and walks 32-key tiles at kv0.
// q rows are local [0,Tq); their GLOBAL positions are +qoff (context
// parallelism: K/V cover the full sequence [0,Tk), Q is this rank's shard).
__device__ __forceinline__ int qmajor_kv_end(bool causal, int q0, int qoff, int Tk) {
  return causal ? min(q0 + qoff + 128, Tk) : Tk;
}
// the wave has at least one visible (q, key) pair in the tile
__device__ __forceinline__ bool qmajor_active(bool causal, int kv0, int qw, int qoff) {
  return !causal || kv0 <= qw + qoff + 31;
}
// the tile crosses the diagonal: only then is the per-element mask needed
__device__ __forceinline__ bool qmajor_diag(bool causal, int kv0, int qw, int qoff) {
  return causal && (kv0 + 31 > qw + qoff);
}

// ===========================================================================
// forward
// grid: T/128 * B*H blocks, mapped to (q block, head) by attn_block_of
// (attn.h); block 256.  Each wave owns 32 q rows.
// q/k/v strided [.., T, 64] slices; out written via its own strides
// (so [B, T, H*64] layout comes out directly); lse2 [BH, T] f32.
// ===========================================================================
template <int MINW, bool KLDS>
__global__ __launch_bounds__(256, MINW) void attn_fwd_kernel(
    const unsigned short* __restrict__ q, const unsigned short* __restrict__ k,
    const unsigned short* __restrict__ v, unsigned short* __restrict__ out,
    float* __restrict__ lse2, int Tq, int Tk, int qoff, int H, int BH, int order,
    float scale, int causal, AttnView qs, AttnView ks, AttnView vs, AttnView os) {
  __shared__ unsigned short vt[64 * TPAD + (KLDS ? 32 * KPAD : 0)];
  unsigned short* klds = vt + 64 * TPAD;  // [32][KPAD] row-major K tile
  const AttnBlock wb = attn_block_of(blockIdx.x, Tq >> 7, BH, order);
  const int bh = wb.bh;
  const int b = bh / H, h = bh % H;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int q0 = wb.blk * 128;            // block q range [q0, q0+128)
  const int qw = q0 + wave * 32;          // wave q range  [qw, qw+32)
  const int myq = qw + (lane & 31);       // this lane's q row

  const unsigned short* qp = q + b * qs.B + h * qs.H;
  const unsigned short* kp = k + b * ks.B + h * ks.H;
  const unsigned short* vp = v + b * vs.B + h * vs.H;
  unsigned short* op = out + b * os.B + h * os.H;

  // Q fragments (B-operand): held in regs for the whole kernel
  bf16x8 qf[4];
#pragma unroll
  for (int kt = 0; kt < 4; ++kt) qf[kt] = frag_ld(qp, qs.T, qw, kt * 16, lane);

  float m2 = -INFINITY, l = 0.f;
  f32x16 o[2];
#pragma unroll
  for (int i = 0; i < 16; ++i) { o[0][i] = 0.f; o[1][i] = 0.f; }
  f32x16 zc;  // persistent zero C operand (keeps per-tile init out of the loop)
#pragma unroll
  for (int i = 0; i < 16; ++i) zc[i] = 0.f;

  const float s2scale = scale * LOG2E;
  const int kv_end = qmajor_kv_end(causal, q0, qoff, Tk);
  const int st_off = rowimg_st_off(), fr_off = rowimg_frag_off(lane);  // KLDS

  // prefetch pipeline: tile t's K fragments + V staging rows load during
  // tile t-1's MFMA cluster (T14) — the per-iteration global latency was
  // the dominant cost of the unpipelined version.  Source addresses are
  // pointer-bumped (+= 32 rows per tile), never rebuilt.
  const unsigned short* kfp = frag_base(kp, ks.T, 0, lane);
  const unsigned short* ksp = stage_base(kp, ks.T, 0);   // KLDS path
  const unsigned short* vsp = stage_base(vp, vs.T, 0);
  const long long kstep = 32 * ks.T, vstep = 32 * vs.T;
  bf16x8 kf_n[4];
  s16x8 v_n = stage_at(vsp);
  s16x8 k_n = {0, 0, 0, 0, 0, 0, 0, 0};
  if constexpr (KLDS) {
    k_n = stage_at(ksp);
  } else {
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) kf_n[kt] = frag_at(kfp, kt);
  }

  for (int kv0 = 0; kv0 < kv_end; kv0 += 32) {
    // cooperative V^T (+ row-major K) staging: write the prefetched rows
    __syncthreads();
    stage_wr(vt, v_n);
    if constexpr (KLDS) rowimg_st(klds, st_off, k_n);
    __syncthreads();

    bf16x8 kf_c[4];
    if constexpr (KLDS) {
      // shared K fragments from the LDS row image
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) kf_c[kt] = frag_at(klds + fr_off, kt);
    } else {
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) kf_c[kt] = kf_n[kt];
    }
    if (kv0 + 32 < kv_end) {
      vsp += vstep;
      v_n = stage_at(vsp);
      if constexpr (KLDS) {
        ksp += kstep;
        k_n = stage_at(ksp);
      } else {
        kfp += kstep;
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) kf_n[kt] = frag_at(kfp, kt);
      }
    }

    if (qmajor_active(causal, kv0, qw, qoff)) {
      // S^T[key][q] = sum_d K[key][d] Q[q][d]  (first mfma takes the
      // persistent zero C — no per-tile accumulator re-init)
      f32x16 s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf_c[0], qf[0], zc, 0, 0, 0);
#pragma unroll
      for (int kt = 1; kt < 4; ++kt) {
        s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf_c[kt], qf[kt], s, 0, 0, 0);
      }
      // scale to base-2; causal mask only on the diagonal tile
      const bool diag = qmajor_diag(causal, kv0, qw, qoff);
      float ps[16];
      float pmax = -INFINITY;
      if (diag) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          int key = kv0 + drow(r, lane);
          float x = s[r] * s2scale;
          if (key > myq + qoff) x = -INFINITY;
          ps[r] = x;
          pmax = fmaxf(pmax, x);
        }
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          ps[r] = s[r] * s2scale;
          pmax = fmaxf(pmax, ps[r]);
        }
      }
      pmax = fmaxf(pmax, __shfl_xor(pmax, 32, 64));
      // defer-max (guide T13, THR=8 in base-2): skip the O/l rescale
      // when no row max grew past the threshold; P <= 2^8 which bf16
      // accumulation tolerates.  The rescale path is also what forces
      // the O accumulator out of AGPRs — skipping it most tiles is the
      // main VALU saving.
      if (!__all(pmax - m2 <= 8.0f)) {
        float mnew = fmaxf(m2, pmax);
        float alpha = __builtin_amdgcn_exp2f(m2 - mnew);  // exp2(-inf)=0 first tile
        l *= alpha;
        m2 = mnew;
#pragma unroll
        for (int i = 0; i < 16; ++i) { o[0][i] *= alpha; o[1][i] *= alpha; }
      }
      float psum = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        ps[r] = __builtin_amdgcn_exp2f(ps[r] - m2);  // exp2(-inf - m2) = 0
        psum += ps[r];
      }
      psum += __shfl_xor(psum, 32, 64);
      l += psum;
      // P fragments (B-operand, k = key): two 16-key blocks
      bf16x8 pf0 = relayout8(ps);
      bf16x8 pf1 = relayout8(ps + 8);
      // O^T[d][q] += V^T · P : A from vt
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) tmfma2(vt, mt, lane, pf0, pf1, o[mt]);
    }
  }

  // epilogue: normalize and store out[q][d] (scattered: lane owns col q)
  float inv = (l > 0.f) ? 1.0f / l : 0.f;
  if (myq < Tq) {
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) drow_st(op + (long long)myq * os.T, mt, lane, o[mt] * inv);
    if (lane < 32) lse2[(long long)bh * Tq + myq] = m2 + __log2f(l);
  }
}

// ===========================================================================
// delta[row] = sum_d dout[row][d] * out[row][d]   (one wave per row)
// ===========================================================================
__global__ void attn_delta_kernel(
    const unsigned short* __restrict__ dout, const unsigned short* __restrict__ out,
    float* __restrict__ delta, long long nrows, int T, int H, AttnView dos,
    AttnView os) {
  // 4 rows per wave, s16x4 (8B) loads per lane: lane l covers row l>>4,
  // elems (l&15)*4 .. +4 (D = 64)
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int sub = lane >> 4;       // row within the wave's group of 4
  const int d0 = (lane & 15) * 4;
  const long long row = ((long long)blockIdx.x * 4 + wave) * 4 + sub;
  if (row >= nrows) return;
  const int t = (int)(row % T);
  const int bh = (int)(row / T);
  const int b = bh / H, h = bh % H;
  const unsigned short* dp = dout + b * dos.B + h * dos.H + (long long)t * dos.T + d0;
  const unsigned short* op = out + b * os.B + h * os.H + (long long)t * os.T + d0;
  s16x4 dv = *reinterpret_cast<const s16x4*>(dp);
  s16x4 ov = *reinterpret_cast<const s16x4*>(op);
  float acc = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    acc += bf16_to_f32((unsigned short)dv[j]) * bf16_to_f32((unsigned short)ov[j]);
  // reduce within each 16-lane group
#pragma unroll
  for (int off = 1; off < 16; off <<= 1) acc += __shfl_xor(acc, off, 64);
  if ((lane & 15) == 0) delta[row] = acc;
}

// ===========================================================================
// backward dQ: block owns a 128-row q tile (wave per 32 rows), loops kv.
// dQ^T[d][q] += K^T[d][key] · g^T[key][q],
//   g^T = scale * P^T ⊙ (dP^T - delta[q]),  P^T = exp2(s2 - lse2[q])
//
// PIPE = true is the shipped form: a cross-tile pipeline — dQ MFMAs of
// tile i, barrier, then the S/dP MFMAs for tile i+1 from the freshly
// staged LDS row images, with tile i+2's staging loads in flight.
// PIPE = false is the non-pipelined form for the 4-waves/SIMD point
// (QN_ATTN_DQ_OCC=4), the same trade as in attn_bwd_dkv_kernel: the S/dP
// chains become transient inside the tile (no cross-tile pipelining), the
// softmax runs 8 values at a time, staging loads issue after the tile's
// MFMAs, and the extra resident wave hides the latency the in-wave overlap
// used to.  The pipelined <3> form needs 162 VGPRs; instantiating it at 4
// waves spills 22.
// ===========================================================================
template <int MINW, bool PIPE>
__global__ __launch_bounds__(256, MINW) void attn_bwd_dq_kernel(
    const unsigned short* __restrict__ q, const unsigned short* __restrict__ k,
    const unsigned short* __restrict__ v, const unsigned short* __restrict__ dout,
    const float* __restrict__ lse2, const float* __restrict__ delta,
    unsigned short* __restrict__ dq, int Tq, int Tk, int qoff, int H, int BH,
    int order, float scale, int causal, AttnView qs, AttnView ks, AttnView vs,
    AttnView dos, AttnView dqs) {
  // double-buffered K^T tile + row-major K/V images: the shared fragment
  // source for the S/dP MFMAs (replaces 4x-redundant per-wave global
  // fragment loads)
  __shared__ unsigned short kt_lds[2][64 * TPAD];
  __shared__ unsigned short krow_l[2][32 * KPAD];
  __shared__ unsigned short vrow_l[2][32 * KPAD];
  const AttnBlock wb = attn_block_of(blockIdx.x, Tq >> 7, BH, order);
  const int bh = wb.bh;
  const int b = bh / H, h = bh % H;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int q0 = wb.blk * 128;
  const int qw = q0 + wave * 32;
  const int myq = qw + (lane & 31);

  const unsigned short* qp = q + b * qs.B + h * qs.H;
  const unsigned short* kp = k + b * ks.B + h * ks.H;
  const unsigned short* vp = v + b * vs.B + h * vs.H;
  const unsigned short* dop = dout + b * dos.B + h * dos.H;
  unsigned short* dqp = dq + b * dqs.B + h * dqs.H;

  bf16x8 qf[4], dof[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    qf[t] = frag_ld(qp, qs.T, qw, t * 16, lane);
    dof[t] = frag_ld(dop, dos.T, qw, t * 16, lane);
  }
  const float my_lse = lse2[(long long)bh * Tq + min(myq, Tq - 1)];
  const float my_delta = delta[(long long)bh * Tq + min(myq, Tq - 1)];
  const float s2scale = scale * LOG2E;

  f32x16 dqa[2], zc;
#pragma unroll
  for (int i = 0; i < 16; ++i) { dqa[0][i] = 0.f; dqa[1][i] = 0.f; zc[i] = 0.f; }

  const int kv_end = qmajor_kv_end(causal, q0, qoff, Tk);
  const unsigned short* ksp = stage_base(kp, ks.T, 0);
  const unsigned short* vsp = stage_base(vp, vs.T, 0);
  const long long kstep = 32 * ks.T, vstep = 32 * vs.T;
  const int st_off = rowimg_st_off(), fr_off = rowimg_frag_off(lane);

  // prologue: stage tile 0 (Kt transposed + K/V row images)
  {
    s16x8 k0 = stage_at(ksp);
    s16x8 v0 = stage_at(vsp);
    stage_wr(kt_lds[0], k0);
    rowimg_st(krow_l[0], st_off, k0);
    rowimg_st(vrow_l[0], st_off, v0);
  }
  // PIPE: tile 1's staging rows, prefetched across tile 0's compute
  s16x8 kst_n = {0, 0, 0, 0, 0, 0, 0, 0}, vst_n = kst_n;
  if constexpr (PIPE) {
    if (32 < kv_end) {
      kst_n = stage_at(ksp + kstep);
      vst_n = stage_at(vsp + vstep);
    }
  }
  __syncthreads();  // buf0 visible
  f32x16 s, dp_;
  if constexpr (PIPE) sdp_chain(&krow_l[0][fr_off], &vrow_l[0][fr_off], qf, dof, zc, s, dp_);

  int cur = 0;
  for (int kv0 = 0; kv0 < kv_end; kv0 += 32) {
    const bool have_next = kv0 + 32 < kv_end;
    const bool active = qmajor_active(causal, kv0, qw, qoff);

    bf16x8 gf0, gf1;
    if (active) {
      // !PIPE: transient S/dP chains for THIS tile
      if constexpr (!PIPE)
        sdp_chain(&krow_l[cur][fr_off], &vrow_l[cur][fr_off], qf, dof, zc, s, dp_);
      const bool diag = qmajor_diag(causal, kv0, qw, qoff);
      if constexpr (PIPE) {
        float g[16];
        if (diag) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            int key = kv0 + drow(r, lane);
            float p = (key > myq + qoff) ? 0.f
                                         : __builtin_amdgcn_exp2f(s[r] * s2scale - my_lse);
            g[r] = scale * p * (dp_[r] - my_delta);
          }
        } else {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            float p = __builtin_amdgcn_exp2f(s[r] * s2scale - my_lse);
            g[r] = scale * p * (dp_[r] - my_delta);
          }
        }
        gf0 = relayout8(g);
        gf1 = relayout8(g + 8);
      } else {
        // softmax half at a time (8-float g liveness)
#pragma unroll
        for (int half = 0; half < 2; ++half) {
          float g[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            int r = half * 8 + j;
            float p;
            if (diag) {
              int key = kv0 + drow(r, lane);
              p = (key > myq + qoff)
                      ? 0.f
                      : __builtin_amdgcn_exp2f(s[r] * s2scale - my_lse);
            } else {
              p = __builtin_amdgcn_exp2f(s[r] * s2scale - my_lse);
            }
            g[j] = scale * p * (dp_[r] - my_delta);
          }
          if (half == 0) gf0 = relayout8(g); else gf1 = relayout8(g);
        }
      }
    }

    if constexpr (PIPE) {
      if (have_next) {
        stage_wr(kt_lds[cur ^ 1], kst_n);
        rowimg_st(krow_l[cur ^ 1], st_off, kst_n);
        rowimg_st(vrow_l[cur ^ 1], st_off, vst_n);
        ksp += kstep;
        vsp += vstep;
        if (kv0 + 64 < kv_end) {
          kst_n = stage_at(ksp + kstep);
          vst_n = stage_at(vsp + vstep);
        }
      }
    }

    if (active) {
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) tmfma2(kt_lds[cur], mt, lane, gf0, gf1, dqa[mt]);
    }

    if constexpr (!PIPE) {
      if (have_next) {
        // stage tile i+1 (loads issued after the MFMAs — registers are
        // not live across compute; the 4th wave hides the latency)
        kst_n = stage_at(ksp + kstep);
        vst_n = stage_at(vsp + vstep);
        stage_wr(kt_lds[cur ^ 1], kst_n);
        rowimg_st(krow_l[cur ^ 1], st_off, kst_n);
        rowimg_st(vrow_l[cur ^ 1], st_off, vst_n);
        ksp += kstep;
        vsp += vstep;
      }
    }
    __syncthreads();  // buf[cur^1] writes visible; buf[cur] reads done
    if constexpr (PIPE) {
      if (have_next)
        sdp_chain(&krow_l[cur ^ 1][fr_off], &vrow_l[cur ^ 1][fr_off], qf, dof, zc, s, dp_);
    }
    cur ^= 1;
  }

  if (myq < Tq) {
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) drow_st(dqp + (long long)myq * dqs.T, mt, lane, dqa[mt]);
  }
}

// ===========================================================================
// backward dK/dV: block owns a 128-key kv tile (wave per 32 keys),
// loops q tiles.  Mirrored orientation: lane owns a KEY column.
//   S[q][key], P = exp2(s2 - lse2[q]); dP[q][key] = dO·V^T
//   dV^T[d][key] += dO^T[d][q] · P[q][key]
//   dK^T[d][key] += Q^T[d][q] · g[q][key]
//
// PIPE = true is the shipped form: the loop is software-pipelined across
// q-tiles — the S/dP MFMAs of tile i+1 interleave with the dV/dK MFMAs of
// tile i (all 6 accumulator chains independent), with tile i+2's staging
// loads in flight.  That needs ~205 VGPRs — 2 waves/SIMD; instantiating
// IT at 3 waves spills 39 regs (offline dump, profiles/kernel_resources.md).
// PIPE = false is the non-pipelined form for the 3-waves/SIMD occupancy
// point (QN_ATTN_DKV_OCC=3): the whole tile-i chain (S/dP -> softmax ->
// dV/dK) runs inside one iteration so s/dp are TRANSIENT, the softmax
// runs 8 values at a time, and the staging loads issue after the tile's
// MFMAs, trading in-wave MFMA overlap for one extra resident wave to hide
// the latency instead.  Same math, same LDS layout, ONE barrier per tile
// in both forms.  Numerics gate for every instantiation:
// tests/test_attention_variants_gpu.py.
// ===========================================================================
template <int MINW, bool PIPE>
__global__ __launch_bounds__(256, MINW) void attn_bwd_dkv_kernel(
    const unsigned short* __restrict__ q, const unsigned short* __restrict__ k,
    const unsigned short* __restrict__ v, const unsigned short* __restrict__ dout,
    const float* __restrict__ lse2, const float* __restrict__ delta,
    unsigned short* __restrict__ dk, unsigned short* __restrict__ dv,
    int Tq, int Tk, int qoff, int H, int BH, int order, float scale, int causal,
    AttnView qs, AttnView ks, AttnView vs, AttnView dos, AttnView dks,
    AttnView dvs) {
  // double-buffered transpose tiles + per-tile lse/delta rows
  __shared__ unsigned short dot_lds[2][64 * TPAD];
  __shared__ unsigned short qt_lds[2][64 * TPAD];
  // row-major q/dO tiles: shared fragment source for the S/dP MFMAs
  // (replaces 4x-redundant per-wave global fragment loads — the fwd
  // K-through-LDS result, +40% there)
  __shared__ unsigned short qrow[2][32 * KPAD];
  __shared__ unsigned short dorow[2][32 * KPAD];
  __shared__ alignas(16) float lse_t[2][32];
  __shared__ alignas(16) float del_t[2][32];
  const AttnBlock wb = attn_block_of(blockIdx.x, Tk >> 7, BH, order);
  const int bh = wb.bh;
  const int b = bh / H, h = bh % H;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int kv0b = wb.blk * 128;
  const int kw = kv0b + wave * 32;
  const int mykey = kw + (lane & 31);

  const unsigned short* qp = q + b * qs.B + h * qs.H;
  const unsigned short* kp = k + b * ks.B + h * ks.H;
  const unsigned short* vp = v + b * vs.B + h * vs.H;
  const unsigned short* dop = dout + b * dos.B + h * dos.H;
  unsigned short* dkp = dk + b * dks.B + h * dks.H;
  unsigned short* dvp = dv + b * dvs.B + h * dvs.H;

  bf16x8 kf[4], vf[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    kf[t] = frag_ld(kp, ks.T, kw, t * 16, lane);
    vf[t] = frag_ld(vp, vs.T, kw, t * 16, lane);
  }
  const float s2scale = scale * LOG2E;

  f32x16 dka[2], dva[2], zc;
#pragma unroll
  for (int i = 0; i < 16; ++i) { dka[0][i] = dka[1][i] = dva[0][i] = dva[1][i] = 0.f; zc[i] = 0.f; }

  // ---- causal window, key-major loop: block owns keys [kv0b, kv0b+128),
  // wave keys [kw, kw+32), and walks 32-row q tiles at qt0 in LOCAL q
  // space; keys at kv0b are causally visible to local q rows >= kv0b - qoff
  // (qoff and kv0b are both multiples of 128)
  const int q_start = causal ? max(kv0b - qoff, 0) : 0;
  // pointer-bumped sources
  const unsigned short* qsp = stage_base(qp, qs.T, q_start);
  const unsigned short* dosp = stage_base(dop, dos.T, q_start);
  const float* lsep = lse2 + (long long)bh * Tq + q_start + threadIdx.x;
  const float* delp = delta + (long long)bh * Tq + q_start + threadIdx.x;
  const long long qstep = 32 * qs.T, dstep = 32 * dos.T;
  const int st_off = rowimg_st_off(), fr_off = rowimg_frag_off(lane);

  // ---- prologue: stage tile 0 into buf0 (transposed + row images) ---------
  {
    s16x8 d0 = stage_at(dosp);
    s16x8 q0 = stage_at(qsp);
    stage_wr(dot_lds[0], d0);
    stage_wr(qt_lds[0], q0);
    rowimg_st(dorow[0], st_off, d0);
    rowimg_st(qrow[0], st_off, q0);
    if (threadIdx.x < 32) {
      lse_t[0][threadIdx.x] = *lsep;
      del_t[0][threadIdx.x] = *delp;
    }
  }
  // PIPE: tile 1's staging rows + lse/del, prefetched across tile 0's compute
  s16x8 dost_n = {0, 0, 0, 0, 0, 0, 0, 0}, qst_n = dost_n;
  float lse_n = 0.f, del_n = 0.f;
  if constexpr (PIPE) {
    if (q_start + 32 < Tq) {
      dost_n = stage_at(dosp + dstep);
      qst_n = stage_at(qsp + qstep);
      if (threadIdx.x < 32) {
        lse_n = lsep[32];
        del_n = delp[32];
      }
    }
  }
  __syncthreads();  // buf0 visible
  f32x16 s, dp_;
  // PIPE: prime s/dp for tile 0 from the LDS row images
  if constexpr (PIPE) sdp_chain(&qrow[0][fr_off], &dorow[0][fr_off], kf, vf, zc, s, dp_);

  int cur = 0;
  for (int qt0 = q_start; qt0 < Tq; qt0 += 32) {
    const bool have_next = qt0 + 32 < Tq;
    // the wave has at least one visible (q, key) pair in the tile
    const bool active = !(causal && qt0 + qoff + 31 < kw);

    // softmax + relayout for tile i.  The 16 lse/delta rows a lane needs
    // are 4 contiguous quadruples (drow: r&3 is the fast index) — 8 vector
    // LDS loads issued together instead of 32 dependent ds_read_b32 round
    // trips (the asm showed 24 full lgkmcnt(0) drains per tile from the
    // scalar form).
    bf16x8 pf0, pf1, gf0, gf1;
    if (active) {
      // !PIPE: S/dP for THIS tile from the row images (transient chains)
      if constexpr (!PIPE)
        sdp_chain(&qrow[cur][fr_off], &dorow[cur][fr_off], kf, vf, zc, s, dp_);
      // the tile crosses the diagonal: only then is the per-element mask needed
      const bool diag = causal && (qt0 + qoff < kw + 31);
      const int lb = (lane >> 5) << 2;
      if constexpr (PIPE) {
        float pv[16], gv[16];
        if (diag) {
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            f32x4 lse4 = *reinterpret_cast<const f32x4*>(&lse_t[cur][lb + g * 8]);
            f32x4 del4 = *reinterpret_cast<const f32x4*>(&del_t[cur][lb + g * 8]);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              int r = g * 4 + j;
              int qrow = drow(r, lane);
              float p = (mykey > qt0 + qoff + qrow)
                            ? 0.f
                            : __builtin_amdgcn_exp2f(s[r] * s2scale - lse4[j]);
              pv[r] = p;
              gv[r] = scale * p * (dp_[r] - del4[j]);
            }
          }
        } else {
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            f32x4 lse4 = *reinterpret_cast<const f32x4*>(&lse_t[cur][lb + g * 8]);
            f32x4 del4 = *reinterpret_cast<const f32x4*>(&del_t[cur][lb + g * 8]);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              int r = g * 4 + j;
              float p = __builtin_amdgcn_exp2f(s[r] * s2scale - lse4[j]);
              pv[r] = p;
              gv[r] = scale * p * (dp_[r] - del4[j]);
            }
          }
        }
        pf0 = relayout8(pv); pf1 = relayout8(pv + 8);
        gf0 = relayout8(gv); gf1 = relayout8(gv + 8);
      } else {
        // HALF at a time: pv/gv live 8 floats each instead of 16 (register
        // pressure — this form trades in-wave ILP for occupancy everywhere)
#pragma unroll
        for (int half = 0; half < 2; ++half) {
          float pv[8], gv[8];
#pragma unroll
          for (int g = 0; g < 2; ++g) {
            const int gg = half * 2 + g;
            f32x4 lse4 = *reinterpret_cast<const f32x4*>(&lse_t[cur][lb + gg * 8]);
            f32x4 del4 = *reinterpret_cast<const f32x4*>(&del_t[cur][lb + gg * 8]);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              int r = gg * 4 + j;
              float p;
              if (diag) {
                int qrow_ = drow(r, lane);
                p = (mykey > qt0 + qoff + qrow_)
                        ? 0.f
                        : __builtin_amdgcn_exp2f(s[r] * s2scale - lse4[j]);
              } else {
                p = __builtin_amdgcn_exp2f(s[r] * s2scale - lse4[j]);
              }
              pv[g * 4 + j] = p;
              gv[g * 4 + j] = scale * p * (dp_[r] - del4[j]);
            }
          }
          if (half == 0) { pf0 = relayout8(pv); gf0 = relayout8(gv); }
          else           { pf1 = relayout8(pv); gf1 = relayout8(gv); }
        }
      }
    }

    // PIPE: stage tile i+1 into the other buffer (its last readers finished
    // before the barrier of the previous iteration)
    if constexpr (PIPE) {
      if (have_next) {
        stage_wr(dot_lds[cur ^ 1], dost_n);
        stage_wr(qt_lds[cur ^ 1], qst_n);
        rowimg_st(dorow[cur ^ 1], st_off, dost_n);
        rowimg_st(qrow[cur ^ 1], st_off, qst_n);
        if (threadIdx.x < 32) {
          lse_t[cur ^ 1][threadIdx.x] = lse_n;
          del_t[cur ^ 1][threadIdx.x] = del_n;
        }
        // issue tile i+2 staging prefetch
        qsp += qstep; dosp += dstep;
        lsep += 32; delp += 32;
        if (qt0 + 64 < Tq) {
          dost_n = stage_at(dosp + dstep);
          qst_n = stage_at(qsp + qstep);
          if (threadIdx.x < 32) {
            lse_n = lsep[32];
            del_n = delp[32];
          }
        }
      }
    }

    // dV/dK MFMAs for tile i (LDS buf[cur]) — under PIPE they interleave
    // with the S/dP MFMAs for tile i+1 below (independent accumulators)
    if (active) {
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) {
        tmfma2(dot_lds[cur], mt, lane, pf0, pf1, dva[mt]);
        tmfma2(qt_lds[cur], mt, lane, gf0, gf1, dka[mt]);
      }
    }

    if constexpr (!PIPE) {
      if (have_next) {
        // stage tile i+1 into the other buffer.  Loads are issued HERE,
        // after the tile's MFMAs, so their registers are not live across
        // the compute — at 3 waves/SIMD the other waves' compute covers
        // the load latency that in-tile overlap covered at 2 waves.
        dost_n = stage_at(dosp + dstep);
        qst_n = stage_at(qsp + qstep);
        stage_wr(dot_lds[cur ^ 1], dost_n);
        stage_wr(qt_lds[cur ^ 1], qst_n);
        rowimg_st(dorow[cur ^ 1], st_off, dost_n);
        rowimg_st(qrow[cur ^ 1], st_off, qst_n);
        if (threadIdx.x < 32) {
          lse_t[cur ^ 1][threadIdx.x] = lsep[32];
          del_t[cur ^ 1][threadIdx.x] = delp[32];
        }
        qsp += qstep; dosp += dstep;
        lsep += 32; delp += 32;
      }
    }
    __syncthreads();  // buf[cur^1] writes visible; buf[cur] reads done
    if constexpr (PIPE) {
      // S/dP for tile i+1 from the freshly staged row images — the next
      // iteration's writes target buf[cur], whose readers all finished
      // before the barrier above
      if (have_next)
        sdp_chain(&qrow[cur ^ 1][fr_off], &dorow[cur ^ 1][fr_off], kf, vf, zc, s, dp_);
    }
    cur ^= 1;
  }

  if (mykey < Tk) {
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
      drow_st(dkp + (long long)mykey * dks.T, mt, lane, dka[mt]);
      drow_st(dvp + (long long)mykey * dvs.T, mt, lane, dva[mt]);
    }
  }
}

// ---- launchers (interface: attn.h) ----------------------------------------
// Every knob is read once per process, on the first launch that needs it.
static const char* knob(const char* name, const char* dflt) {
  const char* e = std::getenv(name);
  return e ? e : dflt;
}

// QN_ATTN_ORDER: balanced (default) spreads the causal row blocks evenly
// over the XCDs, heaviest first; linear is the dim3(T/128, B*H) order
// (attn.h: attn_block_of).  Outputs are bit-identical either way.
static int block_order(const AttnArgs& a, bool key_major) {
  static const bool balanced = strcmp(knob("QN_ATTN_ORDER", "balanced"), "linear") != 0;
  return attn_order_for(balanced, a.causal != 0, key_major);
}

void attn_fwd_launch(const AttnArgs& a, hipStream_t stream) {
  static const int occ = atoi(knob("QN_ATTN_FWD_OCC", "3"));
  // default ON: fwd 66.8->47.9 us (r2); only a leading '0' turns it off
  static const bool klds = knob("QN_ATTN_KLDS", "1")[0] != '0';
  auto kern = occ >= 4 ? (klds ? attn_fwd_kernel<4, true> : attn_fwd_kernel<4, false>)
                       : (klds ? attn_fwd_kernel<3, true> : attn_fwd_kernel<3, false>);
  const int BH = a.B * a.H;
  hipLaunchKernelGGL(kern, dim3(a.Tq / 128 * BH), dim3(256), 0, stream,
                     a.q.ptr, a.k.ptr, a.v.ptr, a.out.ptr, a.lse2, a.Tq, a.Tk,
                     a.q_offset, a.H, BH, block_order(a, false), a.scale,
                     a.causal, a.q.st, a.k.st, a.v.st, a.out.st);
}

void attn_delta_launch(const AttnArgs& a, hipStream_t stream) {
  long long rows = (long long)a.B * a.H * a.Tq;
  hipLaunchKernelGGL(attn_delta_kernel, dim3((unsigned)((rows + 15) / 16)),
                     dim3(256), 0, stream, a.dout.ptr, a.out.ptr, a.delta, rows,
                     a.Tq, a.H, a.dout.st, a.out.st);
}

void attn_bwd_dq_launch(const AttnArgs& a, hipStream_t stream) {
  // A/B r2: 3 waves/SIMD = bwd 279.8 -> 265.2 us; 4 = the non-pipelined form
  static const int occ = atoi(knob("QN_ATTN_DQ_OCC", "3"));
  auto kern = occ >= 4   ? attn_bwd_dq_kernel<4, false>
              : occ >= 3 ? attn_bwd_dq_kernel<3, true>
                         : attn_bwd_dq_kernel<2, true>;
  const int BH = a.B * a.H;
  hipLaunchKernelGGL(kern, dim3(a.Tq / 128 * BH), dim3(256), 0, stream,
                     a.q.ptr, a.k.ptr, a.v.ptr, a.dout.ptr, a.lse2, a.delta,
                     a.dq.ptr, a.Tq, a.Tk, a.q_offset, a.H, BH,
                     block_order(a, false), a.scale, a.causal, a.q.st, a.k.st,
                     a.v.st, a.dout.st, a.dq.st);
}

void attn_bwd_dkv_launch(const AttnArgs& a, hipStream_t stream) {
  // 2 = shipped/measured (pipelined); 3 = the non-pipelined form, the r3
  // occupancy candidate — semantics identical either way
  static const int occ = atoi(knob("QN_ATTN_DKV_OCC", "2"));
  auto kern = occ >= 3 ? attn_bwd_dkv_kernel<3, false> : attn_bwd_dkv_kernel<2, true>;
  const int BH = a.B * a.H;
  hipLaunchKernelGGL(kern, dim3(a.Tk / 128 * BH), dim3(256), 0, stream,
                     a.q.ptr, a.k.ptr, a.v.ptr, a.dout.ptr, a.lse2, a.delta,
                     a.dk.ptr, a.dv.ptr, a.Tq, a.Tk, a.q_offset, a.H, BH,
                     block_order(a, true), a.scale, a.causal, a.q.st, a.k.st,
                     a.v.st, a.dout.st, a.dk.st, a.dv.st);
}
