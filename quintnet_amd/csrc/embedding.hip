// Fused token+position embedding lookup (gather) and its scatter-add
// backward (sorted segment sums, atomic-free) for gfx950.  out[n] = wte[ids[n]] + wpe[n % T] in one pass —
// replaces the two eager gathers + add of reference
// utils/GPT2/gpt2_embeddings.py:92-95 (SURVEY.md §2.4 "embedding
// lookup / scatter-add").
#include "common.h"

template <typename T>
__global__ void embedding_pair_fwd_kernel(
    const long long* __restrict__ ids, const T* __restrict__ wte,
    const T* __restrict__ wpe, T* __restrict__ out, long long rows, int Tlen,
    int H) {
  const int lane = threadIdx.x & (QN_WAVE - 1);
  const int wave = threadIdx.x / QN_WAVE;
  const long long row = (long long)blockIdx.x * 4 + wave;
  if (row >= rows) return;
  const long long tok = ids[row];
  const int pos = (int)(row % Tlen);
  const T* te = wte + tok * H;
  const T* pe = wpe + (long long)pos * H;
  T* o = out + row * H;
  if constexpr (sizeof(T) == 2) {
    for (int i = lane * 8; i < H; i += QN_WAVE * 8) {
      s16x8 a = *reinterpret_cast<const s16x8*>(te + i);
      s16x8 b = *reinterpret_cast<const s16x8*>(pe + i);
      s16x8 r;
#pragma unroll
      for (int j = 0; j < 8; ++j)
        r[j] = (short)f32_to_bf16(bf16_to_f32((unsigned short)a[j]) +
                                  bf16_to_f32((unsigned short)b[j]));
      *reinterpret_cast<s16x8*>(o + i) = r;
    }
    for (int i = (H & ~7) + lane; i < H; i += QN_WAVE)
      st_from_f32(o + i, ld_as_f32(te + i) + ld_as_f32(pe + i));
  } else {
    for (int i = lane; i < H; i += QN_WAVE)
      st_from_f32(o + i, ld_as_f32(te + i) + ld_as_f32(pe + i));
  }
}

// backward: dwte[ids[n]] += dout[n]; dwpe[n % T] += dout[n].  No atomics —
// every sum is added in one fixed order, so the grads are bit-reproducible
// run to run.
//
// dwte: the caller passes the ids STABLY SORTED (sorted_ids) with the
// original row of each entry (perm), so a token's rows form one run in
// ascending row order.  The sorted positions are cut into chunks of EMB_CH;
// one wave per (chunk, 128-column tile) walks its chunk, so the work per
// wave is the same whatever the token distribution (a padding token that
// fills 10^4 rows is 10^4/EMB_CH waves, not one).  A run that lies inside a
// chunk is stored straight to dwte.  A run that crosses chunk borders
// leaves at most two partials per chunk in part[chunk][2][H]:
//   [0] the rows of the run that continues from the previous chunk,
//   [1] the rows of a run that starts in this chunk and continues past it.
// embedding_dwte_fold_kernel then adds, for each run head that continues,
// [1] of its chunk and [0] of the following chunks in ascending order.
// dwte is zero-initialised by the caller (tokens that do not occur keep 0).
constexpr int EMB_CH = 16;           // sorted positions per wave
constexpr int EMB_TW = 2 * QN_WAVE;  // columns per wave (2 per lane)

long long embedding_bwd_chunks(long long rows) {
  return (rows + EMB_CH - 1) / EMB_CH;
}

template <typename T>
__global__ void embedding_dwte_chunk_kernel(
    const long long* __restrict__ sorted_ids, const long long* __restrict__ perm,
    const T* __restrict__ dout, float* __restrict__ dwte,
    float* __restrict__ part, long long rows, long long vocab, int H) {
  const int lane = threadIdx.x & (QN_WAVE - 1);
  const int wave = threadIdx.x / QN_WAVE;
  const long long k = (long long)blockIdx.x * 4 + wave;
  const long long s = k * EMB_CH;
  if (s >= rows) return;
  const long long e = min(s + EMB_CH, rows);
  const int c0 = blockIdx.y * EMB_TW + lane;
  const int c1 = c0 + QN_WAVE;
  const bool cont_in = s > 0 && sorted_ids[s - 1] == sorted_ids[s];
  float* p0 = part + k * 2 * H;
  float* p1 = p0 + H;
  long long cur = sorted_ids[s];
  bool first = true;  // still inside the run that holds position s
  float a0 = 0.f, a1 = 0.f;
  for (long long j = s; j < e; ++j) {
    const long long id = sorted_ids[j];
    if (id != cur) {  // the run of `cur` ended inside this chunk
      float* dst = (first && cont_in) ? p0
                   : (cur >= 0 && cur < vocab) ? dwte + cur * H : nullptr;
      if (dst) {
        if (c0 < H) dst[c0] = a0;
        if (c1 < H) dst[c1] = a1;
      }
      a0 = a1 = 0.f;
      cur = id;
      first = false;
    }
    const long long r = perm[j];
    if (r >= 0 && r < rows) {
      const T* g = dout + r * H;
      if (c0 < H) a0 += ld_as_f32(g + c0);
      if (c1 < H) a1 += ld_as_f32(g + c1);
    }
  }
  const bool cont_out = e < rows && sorted_ids[e] == cur;
  float* dst = (first && cont_in) ? p0
               : cont_out ? p1
               : (cur >= 0 && cur < vocab) ? dwte + cur * H : nullptr;
  if (dst) {
    if (c0 < H) dst[c0] = a0;
    if (c1 < H) dst[c1] = a1;
  }
}

__global__ void embedding_dwte_fold_kernel(
    const long long* __restrict__ sorted_ids, const float* __restrict__ part,
    float* __restrict__ dwte, long long rows, long long vocab, int H) {
  const int lane = threadIdx.x & (QN_WAVE - 1);
  const int wave = threadIdx.x / QN_WAVE;
  const long long k = (long long)blockIdx.x * 4 + wave;
  const long long s = k * EMB_CH;
  if (s >= rows) return;
  const long long e = s + EMB_CH;
  if (e >= rows) return;  // last chunk: nothing continues past it
  const long long tok = sorted_ids[e - 1];
  if (sorted_ids[e] != tok) return;  // no run crosses this chunk's end
  // the run's head lies in an earlier chunk: that chunk's wave folds it
  if (sorted_ids[s] == tok && s > 0 && sorted_ids[s - 1] == tok) return;
  if (tok < 0 || tok >= vocab) return;  // never write out of bounds
  const int c0 = blockIdx.y * EMB_TW + lane;
  const int c1 = c0 + QN_WAVE;
  const float* p1 = part + (k * 2 + 1) * H;
  float a0 = (c0 < H) ? p1[c0] : 0.f;
  float a1 = (c1 < H) ? p1[c1] : 0.f;
  for (long long m = k + 1; m * EMB_CH < rows && sorted_ids[m * EMB_CH] == tok; ++m) {
    const float* p0 = part + m * 2 * H;
    if (c0 < H) a0 += p0[c0];
    if (c1 < H) a1 += p0[c1];
  }
  float* te = dwte + tok * H;
  if (c0 < H) te[c0] = a0;
  if (c1 < H) te[c1] = a1;
}

// dwpe[pos][c] = sum_b dout[b*T + pos][c]: one thread per (pos, c), batch
// rows added in ascending order.  Positions >= T keep the caller's zeros.
template <typename T>
__global__ void embedding_dwpe_kernel(
    const T* __restrict__ dout, float* __restrict__ dwpe, long long batch,
    int Tlen, int H) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long long)Tlen * H) return;
  float acc = 0.f;
  const long long stride = (long long)Tlen * H;
  for (long long b = 0; b < batch; ++b) acc += ld_as_f32(dout + b * stride + idx);
  dwpe[idx] = acc;
}

template <typename T>
void embedding_pair_fwd_launch(const long long* ids, const T* wte, const T* wpe,
                               T* out, long long rows, int Tlen, int H,
                               hipStream_t stream) {
  hipLaunchKernelGGL((embedding_pair_fwd_kernel<T>),
                     dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream,
                     ids, wte, wpe, out, rows, Tlen, H);
}

template <typename T>
void embedding_pair_bwd_launch(const long long* sorted_ids, const long long* perm,
                               const T* dout, float* dwte, float* dwpe,
                               float* part, long long rows, long long vocab,
                               int Tlen, int H, hipStream_t stream) {
  // rows is a multiple of Tlen (ids is [..., Tlen]); dwpe has >= Tlen rows;
  // part holds embedding_bwd_chunks(rows) * 2 * H floats
  if (rows <= 0 || Tlen <= 0 || H <= 0) return;
  const long long chunks = embedding_bwd_chunks(rows);
  const dim3 grid((unsigned)((chunks + 3) / 4), (unsigned)((H + EMB_TW - 1) / EMB_TW));
  hipLaunchKernelGGL((embedding_dwte_chunk_kernel<T>), grid, dim3(256), 0, stream,
                     sorted_ids, perm, dout, dwte, part, rows, vocab, H);
  hipLaunchKernelGGL(embedding_dwte_fold_kernel, grid, dim3(256), 0, stream,
                     sorted_ids, part, dwte, rows, vocab, H);
  const long long n = (long long)Tlen * H;
  hipLaunchKernelGGL((embedding_dwpe_kernel<T>),
                     dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream,
                     dout, dwpe, rows / Tlen, Tlen, H);
}

template void embedding_pair_fwd_launch<float>(const long long*, const float*, const float*, float*, long long, int, int, hipStream_t);
template void embedding_pair_fwd_launch<unsigned short>(const long long*, const unsigned short*, const unsigned short*, unsigned short*, long long, int, int, hipStream_t);
template void embedding_pair_bwd_launch<float>(const long long*, const long long*, const float*, float*, float*, float*, long long, long long, int, int, hipStream_t);
template void embedding_pair_bwd_launch<unsigned short>(const long long*, const long long*, const unsigned short*, float*, float*, float*, long long, long long, int, int, hipStream_t);
