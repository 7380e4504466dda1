"""Causal flash attention per pass at a shape with several blocks per
block slot, where the block order (QN_ATTN_ORDER, csrc/attn.h) shows.

    QN_ATTN_ORDER=linear   python tools/bench_attn_order.py [--batch 32]
    QN_ATTN_ORDER=balanced python tools/bench_attn_order.py [--batch 32]

The knob is read once per process: start one process per value.  Times
fwd, delta + dq, and dkv separately, events around --iters calls after a
warm-up, --repeats windows each; prints one line per pass (microseconds
per call: best window, and all windows to show the spread) and the order
in effect.  bench_attn.py runs B = 8: one block per slot, where the order
cannot matter.  Inputs are views of a packed [B, T, 3*H*64] QKV tensor, as
in the GPT-2 step (--layout bhtd: contiguous [B, H, T, 64]).
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

D = 64


def time_us(fn, iters):
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--heads", type=int, default=12)
    ap.add_argument("--seq", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--layout", choices=("packed", "bhtd"), default="packed")
    args = ap.parse_args()
    assert args.seq % 128 == 0 and args.iters >= 30

    from quintnet_amd import _C

    dev = torch.device("cuda", 0)
    B, H, T = args.batch, args.heads, args.seq
    torch.manual_seed(0)

    def heads(t, off):
        return t[:, :, off:off + H * D].view(B, T, H, D).permute(0, 2, 1, 3)

    if args.layout == "packed":
        qkv = torch.randn(B, T, 3 * H * D, device=dev, dtype=torch.bfloat16)
        dqkv = torch.empty_like(qkv)
        q, k, v = (heads(qkv, i * H * D) for i in range(3))
        dq, dk, dv = (heads(dqkv, i * H * D) for i in range(3))
        out = heads(torch.empty(B, T, H * D, device=dev, dtype=torch.bfloat16), 0)
        dout = heads(torch.randn(B, T, H * D, device=dev, dtype=torch.bfloat16), 0)
    else:
        q, k, v, dout = (torch.randn(B, H, T, D, device=dev, dtype=torch.bfloat16)
                         for _ in range(4))
        out, dq, dk, dv = (torch.empty_like(q) for _ in range(4))
    scale = 1.0 / D ** 0.5
    lse2 = _C.attn_fwd(q, k, v, out, scale, True)
    delta = torch.empty_like(lse2)

    passes = [
        ("fwd", lambda: _C.attn_fwd(q, k, v, out, scale, True)),
        ("delta+dq", lambda: _C.attn_bwd(q, k, v, out, dout, lse2, dq, dk, dv,
                                         scale, True, 0, 1, delta)),
        ("dkv", lambda: _C.attn_bwd(q, k, v, out, dout, lse2, dq, dk, dv,
                                    scale, True, 0, 2, delta)),
    ]
    order = os.environ.get("QN_ATTN_ORDER", "balanced (default)")
    print(f"QN_ATTN_ORDER={order}  B={B} H={H} T={T} causal layout={args.layout} "
          f"blocks={B * H * T // 128}")
    for name, fn in passes:
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        ws = [time_us(fn, args.iters) for _ in range(args.repeats)]
        print(f"{name:9s} {min(ws):8.1f} us/call   windows: "
              + " ".join(f"{w:.1f}" for w in ws))


if __name__ == "__main__":
    main()
