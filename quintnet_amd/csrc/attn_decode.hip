// Fused decode attention over a static KV cache for gfx950: head_dim = 64,
// bf16, 1..8 new query rows per (batch, head).
//
// One call appends the new k/v rows at cache rows [past, past+T) and attends
// query row r (global position past + r) over cache rows [0, past + r].
// `past` is read on the device, so one captured graph stays correct as the
// position advances; the launch geometry depends on (B, H, T, Tmax) only.
//
// Design (guide: cdna_hip_programming.md appendix B "Attention decode
// (single-token)" and the "GEMV / M <= 16" staging row): the op is a
// memory-bound stream over K and V with at most 8 query rows, so there is no
// MFMA and no LDS — K/V go straight to registers with 16-byte loads.
//  * split-KV: the key range is cut into chunks of DEC_CH = 64 keys, one
//    single-wave block per (chunk, batch*head).  All 16 loads of a chunk
//    (8 K + 8 V, 1 KiB per instruction, fully coalesced) are issued before
//    the first use.  A chunk that lies wholly above past + T - 1 writes an
//    empty partial (m = -inf, l = 0) and loads nothing: work follows `past`.
//  * lane = (s, g): g = lane & 7 owns 8 of the 64 head dims, s = lane >> 3
//    is the key within a group of 8; load i covers keys c0 + 8 i + s.  A
//    score is an 8-lane butterfly over g; max / sum / PV reduce over s.
//  * append: the block whose chunk holds position past + r takes that row
//    from k_new / v_new (never from the cache) and stores it to the cache.
//    Rows above past + T - 1 are never read: their loads are redirected to
//    row past + T - 1, whose weight for them is exactly 0.  So no block
//    reads a cache row that another block of the launch writes.
//  * each split writes fp32 partials (m, l, o[64]) per query row; a second
//    small kernel folds them in ascending split order (no atomics, no
//    inter-block hand-off), so the output is bit-identical run to run.
//  * a position outside the cache (past < 0 or past + T > Tmax) appends
//    nothing and yields a zero output; nothing is written out of bounds.
#include "common.h"

constexpr int DEC_D = 64;   // head_dim
constexpr int DEC_CH = 64;  // keys per split (= 8 loads x 8 keys)

struct DecodeStrides {
  long long qB, qH, qT, kB, kH, kT, vB, vH, vT, oB, oH, oT;
};

int attn_decode_splits(int Tmax) { return (Tmax + DEC_CH - 1) / DEC_CH; }

// floats of workspace for one call: o[64] + (m, l) per (bh, split, row)
long long attn_decode_workspace(int B, int H, int T, int Tmax) {
  return (long long)B * H * attn_decode_splits(Tmax) * T * (DEC_D + 2);
}

template <int T>
__global__ __launch_bounds__(QN_WAVE) void attn_decode_split_kernel(
    const unsigned short* __restrict__ q, const unsigned short* __restrict__ k_new,
    const unsigned short* __restrict__ v_new, unsigned short* kc,
    unsigned short* vc, const long long* __restrict__ past_p,
    float* __restrict__ part_o, float* __restrict__ part_ml, int H, int Tmax,
    float scale, long long qB, long long qH, long long qT, long long kB,
    long long kH, long long kT, long long vB, long long vH, long long vT) {
  const int lane = threadIdx.x;
  const int g = lane & 7;
  const int s = lane >> 3;
  const int split = blockIdx.x, nsplit = gridDim.x, bh = blockIdx.y;
  const int b = bh / H, h = bh % H;
  const int c0 = split * DEC_CH;
  const long long pslot = (long long)bh * nsplit + split;
  float* po = part_o + pslot * (T * DEC_D);
  float* pml = part_ml + pslot * (T * 2);

  const long long past64 = *past_p;
  const bool in_range = past64 >= 0 && past64 + T <= (long long)Tmax;
  const int past = in_range ? (int)past64 : 0;
  const int jlast = past + T - 1;  // last cache row any query row sees
  if (!in_range || c0 > jlast) {
    if (lane < T) {
      pml[2 * lane] = -INFINITY;
      pml[2 * lane + 1] = 0.f;
    }
    return;
  }

  unsigned short* kcb = kc + (long long)bh * Tmax * DEC_D;
  unsigned short* vcb = vc + (long long)bh * Tmax * DEC_D;
  const unsigned short* knb = k_new + b * kB + h * kH;
  const unsigned short* vnb = v_new + b * vB + h * vH;

  s16x8 kr[8], vr[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int j = c0 + 8 * i + s;
    const int jc = min(j, jlast);  // c0 <= jc <= jlast < Tmax
    const bool is_new = jc >= past;
    const unsigned short* kp =
        is_new ? knb + (jc - past) * kT + 8 * g : kcb + (long long)jc * DEC_D + 8 * g;
    const unsigned short* vp =
        is_new ? vnb + (jc - past) * vT + 8 * g : vcb + (long long)jc * DEC_D + 8 * g;
    kr[i] = *reinterpret_cast<const s16x8*>(kp);
    vr[i] = *reinterpret_cast<const s16x8*>(vp);
  }
  // append: rows [past, jlast] that fall into this chunk
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int j = c0 + 8 * i + s;
    if (j >= past && j <= jlast) {
      *reinterpret_cast<s16x8*>(kcb + (long long)j * DEC_D + 8 * g) = kr[i];
      *reinterpret_cast<s16x8*>(vcb + (long long)j * DEC_D + 8 * g) = vr[i];
    }
  }

  const unsigned short* qb = q + b * qB + h * qH + 8 * g;
#pragma unroll
  for (int r = 0; r < T; ++r) {
    float qf[8];
    ld8_f32(qb + r * qT, qf);
    float sc[8];
    float m = -INFINITY;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      float d = 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) d += qf[e] * bf16_to_f32((unsigned short)kr[i][e]);
      d += __shfl_xor(d, 1, QN_WAVE);
      d += __shfl_xor(d, 2, QN_WAVE);
      d += __shfl_xor(d, 4, QN_WAVE);
      const int j = c0 + 8 * i + s;
      sc[i] = (j <= past + r) ? d * scale : -INFINITY;
      m = fmaxf(m, sc[i]);
    }
    m = fmaxf(m, __shfl_xor(m, 8, QN_WAVE));
    m = fmaxf(m, __shfl_xor(m, 16, QN_WAVE));
    m = fmaxf(m, __shfl_xor(m, 32, QN_WAVE));
    // a row that sees no key of this chunk: m = -inf, every p = 0
    const float ms = (m == -INFINITY) ? 0.f : m;
    float l = 0.f;
    float o[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float p = __expf(sc[i] - ms);
      l += p;
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] += p * bf16_to_f32((unsigned short)vr[i][e]);
    }
#pragma unroll
    for (int off = 8; off < QN_WAVE; off <<= 1) {
      l += __shfl_xor(l, off, QN_WAVE);
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] += __shfl_xor(o[e], off, QN_WAVE);
    }
    if (s == 0) {
      f32x4* dst = reinterpret_cast<f32x4*>(po + r * DEC_D + 8 * g);
      dst[0] = f32x4{o[0], o[1], o[2], o[3]};
      dst[1] = f32x4{o[4], o[5], o[6], o[7]};
    }
    if (lane == 0) {
      pml[2 * r] = m;
      pml[2 * r + 1] = l;
    }
  }
}

// Fold the partials of one query row in ascending split order.  Row r sees
// keys [0, past + r], i.e. splits [0, (past + r) / DEC_CH]; the splits above
// hold empty partials and are not read.
__global__ __launch_bounds__(QN_WAVE) void attn_decode_combine_kernel(
    const float* __restrict__ part_o, const float* __restrict__ part_ml,
    const long long* __restrict__ past_p, unsigned short* __restrict__ out,
    int H, int T, int Tmax, int nsplit, long long oB, long long oH,
    long long oT) {
  const int d = threadIdx.x;
  const int r = blockIdx.x, bh = blockIdx.y;
  const int b = bh / H, h = bh % H;
  unsigned short* op = out + b * oB + h * oH + r * oT + d;
  const long long past64 = *past_p;
  if (past64 < 0 || past64 + T > (long long)Tmax) {
    *op = 0;
    return;
  }
  const int nact = ((int)past64 + r) / DEC_CH + 1;  // <= nsplit
  const float* ml = part_ml + (long long)bh * nsplit * (T * 2) + 2 * r;
  const float* po = part_o + (long long)bh * nsplit * (T * DEC_D) + r * DEC_D + d;
  float M = -INFINITY;
  for (int sp = 0; sp < nact; ++sp) M = fmaxf(M, ml[sp * (T * 2)]);
  float acc = 0.f, L = 0.f;
  for (int sp = 0; sp < nact; ++sp) {
    const float w = __expf(ml[sp * (T * 2)] - M);
    L += ml[sp * (T * 2) + 1] * w;
    acc += po[(long long)sp * (T * DEC_D)] * w;
  }
  *op = f32_to_bf16(acc / L);
}

void attn_decode_launch(const unsigned short* q, const unsigned short* k_new,
                        const unsigned short* v_new, unsigned short* kc,
                        unsigned short* vc, const long long* past, float* work,
                        unsigned short* out, int B, int H, int T, int Tmax,
                        float scale, const DecodeStrides& st,
                        hipStream_t stream) {
  const int nsplit = attn_decode_splits(Tmax);
  float* part_o = work;
  float* part_ml = work + (long long)B * H * nsplit * T * DEC_D;
  dim3 grid(nsplit, B * H);
#define QN_DEC(T_)                                                             \
  case T_:                                                                     \
    hipLaunchKernelGGL((attn_decode_split_kernel<T_>), grid, dim3(QN_WAVE), 0, \
                       stream, q, k_new, v_new, kc, vc, past, part_o, part_ml, \
                       H, Tmax, scale, st.qB, st.qH, st.qT, st.kB, st.kH,      \
                       st.kT, st.vB, st.vH, st.vT);                            \
    break
  switch (T) {
    QN_DEC(1); QN_DEC(2); QN_DEC(3); QN_DEC(4);
    QN_DEC(5); QN_DEC(6); QN_DEC(7); QN_DEC(8);
    default: return;  // the binding rejects T outside 1..8
  }
#undef QN_DEC
  hipLaunchKernelGGL(attn_decode_combine_kernel, dim3(T, B * H), dim3(QN_WAVE),
                     0, stream, part_o, part_ml, past, out, H, T, Tmax, nsplit,
                     st.oB, st.oH, st.oT);
}
