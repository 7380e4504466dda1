// Launch interface of the fused flash attention kernels (attn.hip), shared
// by the kernel TU and bindings.cpp.
#pragma once
#include <hip/hip_runtime.h>

// element strides of one bf16 [B, H, T, 64] view (head_dim contiguous):
// passed by value to the kernels, so the fused-QKV slices and the
// [B, T, H*64] output layout are consumed without transpose copies
struct AttnView {
  long long B, H, T;
};

struct AttnTensor {
  unsigned short* ptr;  // bf16 bits
  AttnView st;
};

// One argument block for all four launchers; each reads the fields of its
// pass and ignores the rest.
struct AttnArgs {
  AttnTensor q;             // [B, H, Tq, 64]
  AttnTensor k, v;          // [B, H, Tk, 64]
  AttnTensor out;           // [B, H, Tq, 64]  fwd: written; delta: read
  AttnTensor dout;          // [B, H, Tq, 64]  backward only, as are:
  AttnTensor dq;            // [B, H, Tq, 64]
  AttnTensor dk, dv;        // [B, H, Tk, 64]
  float* lse2;              // [B*H, Tq]  fwd: written (m2 + log2 l); bwd: read
  float* delta;             // [B*H, Tq]  delta: written; dq, dkv: read
  int B, H, Tq, Tk;         // Tq, Tk multiples of 128
  int q_offset;             // global position of q row 0 (multiple of 128)
  float scale;
  int causal;
};

// ---- block-to-work mapping of the fwd / dq / dkv grids ---------------------
// The three kernels run a 1-D grid of nblk * BH blocks (nblk = T/128 row
// blocks of BH = B*H heads) and turn the linear block id L into the
// (row block, head) they work on.  Workgroups are dealt round-robin over
// the 8 XCDs by linear id, and under the causal mask a row block's work
// grows (q-major: fwd, dq) or shrinks (key-major: dkv) with its index, so
// the order decides how evenly the XCDs are loaded:
//   LINEAR      blk = L % nblk, bh = L / nblk: the order of a
//               dim3(nblk, BH) grid.  At nblk == 8 every block of one XCD
//               has the same blk, i.e. the same weight.
//   HEAVY_HIGH  bh = L % BH, blk = nblk-1 - L / BH   (causal fwd, dq)
//   HEAVY_LOW   bh = L % BH, blk = L / BH            (causal dkv)
//               consecutive L are consecutive heads of one row block, so
//               every XCD gets an equal share of each weight, heaviest
//               first; with BH % 8 == 0 a head's blocks share one XCD (and
//               its L2 copy of that head's K/V).
// A block's arithmetic does not depend on L: every order gives the same bits.
enum AttnOrder { ATTN_ORDER_LINEAR = 0, ATTN_ORDER_HEAVY_HIGH = 1, ATTN_ORDER_HEAVY_LOW = 2 };

struct AttnBlock {
  int blk, bh;
};

// bijection [0, nblk*BH) -> [0, nblk) x [0, BH) for every nblk, BH >= 1;
// one integer division (L and the arguments are wave-uniform: scalar code)
__host__ __device__ inline AttnBlock attn_block_of(unsigned L, int nblk, int BH, int order) {
  const unsigned d = order == ATTN_ORDER_LINEAR ? (unsigned)nblk : (unsigned)BH;
  const int hi = (int)(L / d), lo = (int)(L - (unsigned)hi * d);
  if (order == ATTN_ORDER_LINEAR) return {lo, hi};
  return {order == ATTN_ORDER_HEAVY_HIGH ? nblk - 1 - hi : hi, lo};
}

// the order a launch uses: balanced (QN_ATTN_ORDER, default) only changes
// causal launches — without the mask all blocks weigh the same
inline int attn_order_for(bool balanced, bool causal, bool key_major) {
  if (!balanced || !causal) return ATTN_ORDER_LINEAR;
  return key_major ? ATTN_ORDER_HEAVY_LOW : ATTN_ORDER_HEAVY_HIGH;
}

void attn_fwd_launch(const AttnArgs& a, hipStream_t stream);
void attn_delta_launch(const AttnArgs& a, hipStream_t stream);   // needs out, dout
void attn_bwd_dq_launch(const AttnArgs& a, hipStream_t stream);  // after delta
void attn_bwd_dkv_launch(const AttnArgs& a, hipStream_t stream);  // after delta
