// Fused LayerNorm fwd/bwd for gfx950 — one wave per row, fp32 accumulate.
// Replaces the implicit eager LayerNorm of the reference.
// Rows are B*T; H ∈ {64, 768, 3072, ...}. bf16 loads vectorized as s16x8
// (guide G13: scalar bf16 ≈2× slower), one pass of sum/sumsq per row.
//
// Backward is two kernels: dx (wave-per-row, no atomics) and a separate
// dw/db column reduction (block-per-column-tile × row-chunks, one
// partial per column per chunk, folded in a fixed order afterwards) —
// the v1 per-element atomic version was 20% of the whole GPT-2 step
// (rocprof, profiles/r01).  For bf16 with 512 <= H <= 1024 one kernel does
// both in a single read of dy and x, with the pair's bits
// (layernorm_bwd_fused_kernel below).
#include "common.h"

// ---------------------------------------------------------------------------
// forward: y = (x - mean) * rstd * w + b ; saves mean, rstd (f32 per row)
// ---------------------------------------------------------------------------
template <typename T, int WPB>
__global__ void layernorm_fwd_kernel(
    const T* __restrict__ x, const T* __restrict__ res,
    const T* __restrict__ w, const T* __restrict__ b,
    T* __restrict__ y, T* __restrict__ sum_out,
    float* __restrict__ mean_out, float* __restrict__ rstd_out,
    int rows, int H, float eps) {
  const int lane = threadIdx.x & (QN_WAVE - 1);
  const int wave = threadIdx.x / QN_WAVE;
  const long long row = (long long)blockIdx.x * WPB + wave;
  if (row >= rows) return;
  const T* xr = x + row * H;
  const T* rr = res ? res + row * H : nullptr;
  T* yr = y + row * H;
  T* sr = sum_out ? sum_out + row * H : nullptr;

  float sum = 0.f, sq = 0.f;
  // cache up to 16 elems/lane in registers (H <= 1024) to avoid re-reads
  float cache[16];
  const bool cached = H <= QN_WAVE * 16;
  const bool vec8 = sizeof(T) == 2 && (H & 7) == 0 && H >= 512;
  if (cached && vec8) {
    // 8-wide bf16 loads (G13); lanes own disjoint 8-elem groups
    int n = 0;
    for (int i = lane * 8; i < H; i += QN_WAVE * 8, n += 8) {
      ld8_f32(reinterpret_cast<const unsigned short*>(xr) + i, cache + n);
      if (rr) {
        float rv[8];
        ld8_f32(reinterpret_cast<const unsigned short*>(rr) + i, rv);
#pragma unroll
        for (int j = 0; j < 8; ++j) cache[n + j] += rv[j];
        if (sr) st8_f32(reinterpret_cast<unsigned short*>(sr) + i, cache + n);
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        sum += cache[n + j];
        sq += cache[n + j] * cache[n + j];
      }
    }
  } else if (cached) {
    int n = 0;
    for (int i = lane; i < H; i += QN_WAVE, ++n) {
      float f = ld_as_f32(xr + i);
      if (rr) {  // fused residual add (SURVEY §2.4 "fused residual-add")
        f += ld_as_f32(rr + i);
        if (sr) st_from_f32(sr + i, f);
      }
      cache[n] = f;
      sum += f; sq += f * f;
    }
  } else {
    for (int i = lane; i < H; i += QN_WAVE) {
      float f = ld_as_f32(xr + i);
      if (rr) {
        f += ld_as_f32(rr + i);
        if (sr) st_from_f32(sr + i, f);
      }
      sum += f; sq += f * f;
    }
  }
  sum = wave_reduce_sum(sum);
  sq = wave_reduce_sum(sq);
  const float mean = sum / H;
  const float var = fmaxf(sq / H - mean * mean, 0.f);
  const float rstd = rsqrtf(var + eps);
  if (lane == 0) { mean_out[row] = mean; rstd_out[row] = rstd; }

  if (cached && vec8) {
    int n = 0;
    for (int i = lane * 8; i < H; i += QN_WAVE * 8, n += 8) {
      float wv[8], bv[8], ov[8];
      ld8_f32(reinterpret_cast<const unsigned short*>(w) + i, wv);
      ld8_f32(reinterpret_cast<const unsigned short*>(b) + i, bv);
#pragma unroll
      for (int j = 0; j < 8; ++j)
        ov[j] = (cache[n + j] - mean) * rstd * wv[j] + bv[j];
      st8_f32(reinterpret_cast<unsigned short*>(yr) + i, ov);
    }
  } else if (cached) {
    int n = 0;
    for (int i = lane; i < H; i += QN_WAVE, ++n) {
      float wi = ld_as_f32(w + i);
      float bi = ld_as_f32(b + i);
      st_from_f32(yr + i, (cache[n] - mean) * rstd * wi + bi);
    }
  } else {
    for (int i = lane; i < H; i += QN_WAVE) {
      float f = ld_as_f32(xr + i);
      if (rr) f += ld_as_f32(rr + i);
      float wi = ld_as_f32(w + i);
      float bi = ld_as_f32(b + i);
      st_from_f32(yr + i, (f - mean) * rstd * wi + bi);
    }
  }
}

// ---------------------------------------------------------------------------
// backward dx (wave per row):
//   xhat = (x - mean) * rstd;  wdy = w * dy
//   dx = (wdy - mean(wdy) - xhat * mean(wdy * xhat)) * rstd
// ---------------------------------------------------------------------------
template <typename T, int WPB>
__global__ void layernorm_bwd_dx_kernel(
    const T* __restrict__ dy, const T* __restrict__ x, const T* __restrict__ w,
    const float* __restrict__ mean_in, const float* __restrict__ rstd_in,
    const T* __restrict__ dsum, T* __restrict__ dx, int rows, int H) {
  const int lane = threadIdx.x & (QN_WAVE - 1);
  const int wave = threadIdx.x / QN_WAVE;
  const long long row = (long long)blockIdx.x * WPB + wave;
  if (row >= rows) return;
  const T* xr = x + row * H;
  const T* dyr = dy + row * H;
  const T* dsr = dsum ? dsum + row * H : nullptr;
  T* dxr = dx + row * H;
  const float mean = mean_in[row], rstd = rstd_in[row];

  float cx[16], cwdy[16];
  const bool cached = H <= QN_WAVE * 16;
  const bool vec8 = sizeof(T) == 2 && (H & 7) == 0 && H >= 512;
  float c1 = 0.f, c2 = 0.f;
  if (cached && vec8) {
    int n = 0;
    for (int i = lane * 8; i < H; i += QN_WAVE * 8, n += 8) {
      float xv[8], wv[8], dv[8];
      ld8_f32(reinterpret_cast<const unsigned short*>(xr) + i, xv);
      ld8_f32(reinterpret_cast<const unsigned short*>(w) + i, wv);
      ld8_f32(reinterpret_cast<const unsigned short*>(dyr) + i, dv);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float xhat = (xv[j] - mean) * rstd;
        float wdy = wv[j] * dv[j];
        cx[n + j] = xhat; cwdy[n + j] = wdy;
        c1 += wdy; c2 += wdy * xhat;
      }
    }
  } else if (cached) {
    int n = 0;
    for (int i = lane; i < H; i += QN_WAVE, ++n) {
      float xhat = (ld_as_f32(xr + i) - mean) * rstd;
      float wdy = ld_as_f32(w + i) * ld_as_f32(dyr + i);
      cx[n] = xhat; cwdy[n] = wdy;
      c1 += wdy; c2 += wdy * xhat;
    }
  } else {
    for (int i = lane; i < H; i += QN_WAVE) {
      float xhat = (ld_as_f32(xr + i) - mean) * rstd;
      float wdy = ld_as_f32(w + i) * ld_as_f32(dyr + i);
      c1 += wdy; c2 += wdy * xhat;
    }
  }
  c1 = wave_reduce_sum(c1) / H;
  c2 = wave_reduce_sum(c2) / H;

  if (cached && vec8) {
    int n = 0;
    for (int i = lane * 8; i < H; i += QN_WAVE * 8, n += 8) {
      float ov[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) ov[j] = (cwdy[n + j] - c1 - cx[n + j] * c2) * rstd;
      if (dsr) {
        float dsv[8];
        ld8_f32(reinterpret_cast<const unsigned short*>(dsr) + i, dsv);
#pragma unroll
        for (int j = 0; j < 8; ++j) ov[j] += dsv[j];
      }
      st8_f32(reinterpret_cast<unsigned short*>(dxr) + i, ov);
    }
  } else if (cached) {
    int n = 0;
    for (int i = lane; i < H; i += QN_WAVE, ++n) {
      float v = (cwdy[n] - c1 - cx[n] * c2) * rstd;
      if (dsr) v += ld_as_f32(dsr + i);  // residual-branch grad fused in
      st_from_f32(dxr + i, v);
    }
  } else {
    for (int i = lane; i < H; i += QN_WAVE) {
      float xhat = (ld_as_f32(xr + i) - mean) * rstd;
      float wdy = ld_as_f32(w + i) * ld_as_f32(dyr + i);
      float v = (wdy - c1 - xhat * c2) * rstd;
      if (dsr) v += ld_as_f32(dsr + i);
      st_from_f32(dxr + i, v);
    }
  }
}

// ---------------------------------------------------------------------------
// backward dw/db: column reduction.  grid = (ceil(H/256), ROW_CHUNKS);
// each thread owns one column within its row chunk and writes one partial
// per column per chunk.
// ---------------------------------------------------------------------------
template <typename T>
__global__ void layernorm_bwd_dwdb_kernel(
    const T* __restrict__ dy, const T* __restrict__ x,
    const float* __restrict__ mean_in, const float* __restrict__ rstd_in,
    float* __restrict__ dw, float* __restrict__ db, int rows, int H) {
  const int col = blockIdx.x * blockDim.x + threadIdx.x;
  if (col >= H) return;
  const int r0 = blockIdx.y;
  const int nchunks = gridDim.y;
  float aw = 0.f, ab = 0.f;
  for (long long r = r0; r < rows; r += nchunks) {
    float dyv = ld_as_f32(dy + r * H + col);
    float xhat = (ld_as_f32(x + r * H + col) - mean_in[r]) * rstd_in[r];
    aw += dyv * xhat;
    ab += dyv;
  }
  // dw/db are [nchunks, H] partials, folded over chunks by the caller in a
  // fixed order (no atomics: bit-reproducible run to run)
  dw[(long long)r0 * H + col] = aw;
  db[(long long)r0 * H + col] = ab;
}

int layernorm_bwd_chunks(int rows) { return min(max(rows / 64, 1), 256); }

// ---------------------------------------------------------------------------
// one-pass backward for the fast shape (bf16, H % 8 == 0, 512 <= H <= 1024):
// dx and the dw/db chunk partials from ONE read of dy and x, with the bits of
// the dx + dwdb kernel pair.  Block c owns the dwdb kernel's row chunk c (rows
// c, c + chunks, c + 2*chunks, ...).  Its waves take LNF_WPB of those rows at
// a time: each wave computes dx of its row exactly as layernorm_bwd_dx_kernel
// does and leaves xhat and dy of the row in LDS; then thread t adds the
// staged rows into its column-t accumulators in row order, which is the
// sequence of operations layernorm_bwd_dwdb_kernel runs for that column.
// ---------------------------------------------------------------------------
constexpr int LNF_WPB = 16;     // waves per block = rows staged per round
constexpr int LNF_MAXH = 1024;  // 16 columns per lane, one column per thread

__global__ void __launch_bounds__(LNF_WPB * QN_WAVE)
layernorm_bwd_fused_kernel(
    const unsigned short* __restrict__ dy, const unsigned short* __restrict__ x,
    const unsigned short* __restrict__ w, const float* __restrict__ mean_in,
    const float* __restrict__ rstd_in, const unsigned short* __restrict__ dsum,
    unsigned short* __restrict__ dx, float* __restrict__ dw,
    float* __restrict__ db, int rows, int H) {
  // Results must keep the bits of the two kernels this replaces, so no
  // contraction is left to the optimizer: an fma is written out exactly
  // where their compiled code has one (the dwdb kernel has none).
#pragma clang fp contract(off)
  __shared__ float s_xhat[LNF_WPB][LNF_MAXH];
  __shared__ __attribute__((aligned(16))) unsigned short s_dy[LNF_WPB][LNF_MAXH];
  const int lane = threadIdx.x & (QN_WAVE - 1);
  const int wave = threadIdx.x / QN_WAVE;
  const int nchunks = gridDim.x;
  const int chunk = blockIdx.x;
  // rows of this chunk: chunk + k * nchunks, k < nk
  const int nk = chunk < rows ? (rows - chunk + nchunks - 1) / nchunks : 0;
  const int i0 = lane * 8, i1 = lane * 8 + QN_WAVE * 8;

  float aw = 0.f, ab = 0.f;  // column threadIdx.x
  s16x8 xq[2] = {{0}, {0}}, dq[2] = {{0}, {0}};  // raw x, dy of the wave's row
  if (wave < nk) {
    const long long off = ((long long)chunk + (long long)wave * nchunks) * H;
    if (i0 < H) {
      xq[0] = *reinterpret_cast<const s16x8*>(x + off + i0);
      dq[0] = *reinterpret_cast<const s16x8*>(dy + off + i0);
    }
    if (i1 < H) {
      xq[1] = *reinterpret_cast<const s16x8*>(x + off + i1);
      dq[1] = *reinterpret_cast<const s16x8*>(dy + off + i1);
    }
  }

  for (int k0 = 0; k0 < nk; k0 += LNF_WPB) {
    const int k = k0 + wave;
    // next round's row is loaded ahead of this round's barriers
    s16x8 xn[2] = {xq[0], xq[1]}, dn[2] = {dq[0], dq[1]};
    if (k + LNF_WPB < nk) {
      const long long off =
          ((long long)chunk + (long long)(k + LNF_WPB) * nchunks) * H;
      if (i0 < H) {
        xn[0] = *reinterpret_cast<const s16x8*>(x + off + i0);
        dn[0] = *reinterpret_cast<const s16x8*>(dy + off + i0);
      }
      if (i1 < H) {
        xn[1] = *reinterpret_cast<const s16x8*>(x + off + i1);
        dn[1] = *reinterpret_cast<const s16x8*>(dy + off + i1);
      }
    }
    if (k < nk) {
      const long long row = (long long)chunk + (long long)k * nchunks;
      const unsigned short* dsr = dsum ? dsum + row * H : nullptr;
      unsigned short* dxr = dx + row * H;
      const float mean = mean_in[row], rstd = rstd_in[row];

      float cx[16], cwdy[16];
      float c1 = 0.f, c2 = 0.f;
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        const int i = kk == 0 ? i0 : i1;
        if (i < H) {
          float wv[8];
          ld8_f32(w + i, wv);
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            float xhat = (bf16_to_f32((unsigned short)xq[kk][j]) - mean) * rstd;
            float wdy = wv[j] * bf16_to_f32((unsigned short)dq[kk][j]);
            cx[kk * 8 + j] = xhat; cwdy[kk * 8 + j] = wdy;
            c1 += wdy;
            // as compiled, layernorm_bwd_dx_kernel fuses only the first
            // product of each 8-group into an fma (the other seven are
            // packed multiplies followed by adds)
            c2 = j == 0 ? __builtin_fmaf(wdy, xhat, c2) : c2 + wdy * xhat;
            s_xhat[wave][i + j] = xhat;
          }
          *reinterpret_cast<s16x8*>(&s_dy[wave][i]) = dq[kk];
        }
      }
      c1 = wave_reduce_sum(c1) / H;
      c2 = wave_reduce_sum(c2) / H;

#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        const int i = kk == 0 ? i0 : i1;
        if (i < H) {
          float ov[8];
#pragma unroll
          for (int j = 0; j < 8; ++j)
            ov[j] = __builtin_fmaf(-cx[kk * 8 + j], c2, cwdy[kk * 8 + j] - c1) * rstd;
          if (dsr) {
            float dsv[8];
            ld8_f32(dsr + i, dsv);
#pragma unroll
            for (int j = 0; j < 8; ++j) ov[j] += dsv[j];
          }
          st8_f32(dxr + i, ov);
        }
      }
    }
    __syncthreads();
    // column sums in row order: aw += dy * xhat (rounded product), ab += dy
    const int nact = min(LNF_WPB, nk - k0);
    if ((int)threadIdx.x < H) {
      for (int r = 0; r < nact; ++r) {
        const float d = bf16_to_f32(s_dy[r][threadIdx.x]);
        aw = aw + s_xhat[r][threadIdx.x] * d;
        ab = ab + d;
      }
    }
    __syncthreads();
    xq[0] = xn[0]; xq[1] = xn[1]; dq[0] = dn[0]; dq[1] = dn[1];
  }
  // [chunks, H] partials, the layout layernorm_bwd_dwdb_kernel writes
  if ((int)threadIdx.x < H) {
    dw[(long long)chunk * H + threadIdx.x] = aw;
    db[(long long)chunk * H + threadIdx.x] = ab;
  }
}

bool layernorm_bwd_fused_shape_ok(int H) {
  return (H & 7) == 0 && H >= 512 && H <= LNF_MAXH;
}

// dw, db: [layernorm_bwd_chunks(rows), H] partials each, as for
// layernorm_bwd_launch.  Pointers must be 16-byte aligned.
void layernorm_bwd_fused_launch(const unsigned short* dy, const unsigned short* x,
                                const unsigned short* w, const float* mean,
                                const float* rstd, const unsigned short* dsum,
                                unsigned short* dx, float* dw, float* db,
                                int rows, int H, hipStream_t stream) {
  hipLaunchKernelGGL(layernorm_bwd_fused_kernel, dim3(layernorm_bwd_chunks(rows)),
                     dim3(LNF_WPB * QN_WAVE), 0, stream, dy, x, w, mean, rstd,
                     dsum, dx, dw, db, rows, H);
}

// ---- launchers -------------------------------------------------------------
template <typename T>
void layernorm_fwd_launch(const T* x, const T* res, const T* w, const T* b,
                          T* y, T* sum_out, float* mean, float* rstd, int rows,
                          int H, float eps, hipStream_t stream) {
  constexpr int WPB = 4;
  dim3 grid((rows + WPB - 1) / WPB);
  hipLaunchKernelGGL((layernorm_fwd_kernel<T, WPB>), grid, dim3(WPB * QN_WAVE), 0,
                     stream, x, res, w, b, y, sum_out, mean, rstd, rows, H, eps);
}

template <typename T>
void layernorm_bwd_launch(const T* dy, const T* x, const T* w, const float* mean,
                          const float* rstd, const T* dsum, T* dx, float* dw,
                          float* db, int rows, int H, hipStream_t stream) {
  constexpr int WPB = 4;
  dim3 grid((rows + WPB - 1) / WPB);
  hipLaunchKernelGGL((layernorm_bwd_dx_kernel<T, WPB>), grid, dim3(WPB * QN_WAVE),
                     0, stream, dy, x, w, mean, rstd, dsum, dx, rows, H);
  int colblocks = (H + 255) / 256;
  // dw, db: [layernorm_bwd_chunks(rows), H] partials each
  int chunks = layernorm_bwd_chunks(rows);
  hipLaunchKernelGGL((layernorm_bwd_dwdb_kernel<T>), dim3(colblocks, chunks),
                     dim3(256), 0, stream, dy, x, mean, rstd, dw, db, rows, H);
}

// explicit instantiations
template void layernorm_fwd_launch<float>(const float*, const float*, const float*, const float*,
                                          float*, float*, float*, float*, int, int, float, hipStream_t);
template void layernorm_fwd_launch<unsigned short>(const unsigned short*, const unsigned short*,
                                                   const unsigned short*, const unsigned short*,
                                                   unsigned short*, unsigned short*, float*,
                                                   float*, int, int, float, hipStream_t);
template void layernorm_bwd_launch<float>(const float*, const float*, const float*, const float*,
                                          const float*, const float*, float*, float*, float*, int, int, hipStream_t);
template void layernorm_bwd_launch<unsigned short>(const unsigned short*, const unsigned short*,
                                                   const unsigned short*, const float*, const float*,
                                                   const unsigned short*, unsigned short*, float*, float*, int, int, hipStream_t);
