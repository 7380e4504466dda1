"""Serving decode benchmark: KV-cached autoregressive generation.

GPU:  python bench_decode.py [--batch 1,8,32] [--new 64] [--prompt 128]
                             [--no-fused-attn]
Reports decode tokens/s per batch size (GPT-2 124M, bf16, int8-cache
variant included).
"""
import argparse
import time

import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=str, default="1,8,32")
    ap.add_argument("--new", type=int, default=64)
    ap.add_argument("--prompt", type=int, default=128)
    ap.add_argument("--no-fused-attn", action="store_true",
                    help="graph line with the composed torch attention "
                         "instead of the fused decode-attention kernel")
    args = ap.parse_args()

    from quintnet_amd.models import GPT2Config, GPT2Stage

    dev = torch.device("cuda")
    cfg = GPT2Config(dropout=0.0)
    model = GPT2Stage(cfg, device=dev, dtype=torch.bfloat16).eval()

    from quintnet_amd.models import StaticKVDecoder

    for bs in [int(b) for b in args.batch.split(",")]:
        ids = torch.randint(0, cfg.vocab_size, (bs, args.prompt), device=dev)
        for cache_dtype, tag in [(None, "bf16kv"), ("int8", "int8kv")]:
            # warmup
            model.generate(ids, max_new_tokens=4, cache_dtype=cache_dtype)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = model.generate(ids, max_new_tokens=args.new,
                                 cache_dtype=cache_dtype)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            ntok = (out.shape[1] - args.prompt) * bs
            print(f"bs={bs:<3} {tag}: {ntok / dt:8.1f} tok/s "
                  f"({dt / (out.shape[1] - args.prompt) * 1e3:.2f} ms/token)",
                  flush=True)
        # hipGraph-captured static-cache decode (one replay per token)
        dec = StaticKVDecoder(model, batch=bs,
                              max_len=args.prompt + args.new + 8,
                              fused_attention=False if args.no_fused_attn else None)
        dec.generate(ids, max_new_tokens=4)  # prefill + capture warmup
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = dec.generate(ids, max_new_tokens=args.new)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        ntok = args.new * bs
        # compare a short horizon: random-init logits are tie-heavy in
        # bf16, so long greedy rollouts drift at argmax ties (the graph
        # path is token-exact vs its own eager form — decode_dbg r2)
        ref = model.generate(ids, max_new_tokens=8)
        eq = "ok" if torch.equal(out[:, : args.prompt + 8],
                                 ref[:, : args.prompt + 8]) else "MISMATCH"
        attn = "fused-attn" if dec.fused_attention else "composed-attn"
        print(f"bs={bs:<3} graph : {ntok / dt:8.1f} tok/s "
              f"({dt / args.new * 1e3:.2f} ms/token) {eq} [{attn}]", flush=True)


if __name__ == "__main__":
    main()
