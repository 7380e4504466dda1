"""Decode attention, kernel level: the fused append+attend call
(ops.decode_attention -> csrc/attn_decode.hip) against the composed torch
sequence StaticKVDecoder used before it, both replayed from a captured
graph, single new token.

    python tools/bench_decode_attn.py [--iters 200] [--repeats 3]

H=12, D=64, Tmax=1024, B in {1, 8, 32}, past in {127, 511, 1023}; prints
microseconds per call (one layer's attention) for each, best of --repeats
windows of --iters replays, the two paths alternating.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

H, D, TMAX = 12, 64, 1024


def composed(q, k, v, kc, vc, t0, pos, B, T):
    """The attention part of StaticKVDecoder._block_step, composed form."""
    idx = t0 + torch.arange(T, device=q.device)
    kc.index_copy_(2, idx, k)
    vc.index_copy_(2, idx, v)
    scale = 1.0 / (D ** 0.5)
    scores = torch.matmul(q, kc.transpose(-2, -1)).float() * scale
    qpos = (t0 + torch.arange(T, device=q.device)).view(1, 1, T, 1)
    visible = pos.view(1, 1, 1, -1) <= qpos
    scores = scores.masked_fill(~visible, float("-inf"))
    p = torch.softmax(scores, dim=-1).to(q.dtype)
    out = torch.matmul(p, vc)
    return out.permute(0, 2, 1, 3).reshape(B, T, H * D)


def capture(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g


def time_us(g, iters):
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        g.replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    from quintnet_amd.ops import decode_attention, has_ext

    assert has_ext(), "HIP extension missing"
    dev = torch.device("cuda")
    T = 1
    hl = H * D
    print(f"H={H} D={D} Tmax={TMAX} T={T}: us per call, graph replay, "
          f"best of {args.repeats} x {args.iters}")
    print(f"{'B':>3} {'past':>5} {'composed':>9} {'fused':>9} {'speedup':>8} {'maxdiff':>8}")
    for B in (1, 8, 32):
        torch.manual_seed(B)
        qkv = torch.randn(B, T, 3 * hl, device=dev, dtype=torch.bfloat16)

        def heads(t):
            return t.view(B, T, H, D).permute(0, 2, 1, 3)

        q, k, v = (heads(qkv[:, :, i * hl:(i + 1) * hl]) for i in range(3))
        kc = torch.randn(B, H, TMAX, D, device=dev, dtype=torch.bfloat16)
        vc = torch.randn(B, H, TMAX, D, device=dev, dtype=torch.bfloat16)
        kc2, vc2 = kc.clone(), vc.clone()
        past = torch.zeros((), dtype=torch.long, device=dev)
        pos = torch.arange(TMAX, device=dev)
        buf = torch.empty(B, T, hl, device=dev, dtype=torch.bfloat16)
        res = {}

        def run_fused():
            decode_attention(q, k, v, kc, vc, past, out=heads(buf))

        def run_composed():
            res["out"] = composed(q, k, v, kc2, vc2, past, pos, B, T)

        gf = capture(run_fused)
        gc = capture(run_composed)
        for p in (127, 511, 1023):
            past.fill_(p)
            gf.replay()
            gc.replay()
            torch.cuda.synchronize()
            diff = (buf.float() - res["out"].float()).abs().max().item()
            best_c = best_f = float("inf")
            for _ in range(args.repeats):
                best_c = min(best_c, time_us(gc, args.iters))
                best_f = min(best_f, time_us(gf, args.iters))
            print(f"{B:>3} {p:>5} {best_c:9.2f} {best_f:9.2f} "
                  f"{best_c / best_f:7.2f}x {diff:8.1e}", flush=True)


if __name__ == "__main__":
    main()
