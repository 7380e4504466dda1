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

void attn_fwd_launch(const AttnArgs& a, hipStream_t stream);
void attn_delta_launch(const AttnArgs& a, hipStream_t stream);   // needs out, dout
void attn_bwd_dq_launch(const AttnArgs& a, hipStream_t stream);  // after delta
void attn_bwd_dkv_launch(const AttnArgs& a, hipStream_t stream);  // after delta
