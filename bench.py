#!/usr/bin/env python3
"""Flagship benchmark: GPT-2 (124M) 3D-parallel training step on MI355X.

Driver contract: ``python bench.py --gpus N --steps K --warmup W`` (run
under torch.distributed.run for N>1, one rank per GPU over RCCL).  Does
W untimed warmup steps, times EXACTLY K optimizer steps bracketed by
barrier + torch.cuda.synchronize on both sides, takes the MAX time over
ranks, and rank 0 prints ONE JSON line.

Mesh by GPU count (BASELINE.json configs): 1 → [1,1,1]; 2 → dp2;
4 → dp4; 8 → the named 3D mesh [2,2,2] (dp×tp×pp, 1F1B).  Per-replica
work is fixed (weak scaling): 32 sequences of 1024 tokens per optimizer
step per DP replica (micro 32 × acc 1 at pp=1; micro 8 × acc 4 on the
pipeline mesh), synthetic data, random-init weights, bf16 compute,
ZeRO-1 AdamW.

``--model vit`` benchmarks the ViT-MNIST config instead
(micro 16 × grad_acc 4 = 64 images/replica/step).

A plain run does only what the headline figure needs: set up, warm up,
time the K steps, print the result line.  ``--full`` adds the secondary
measurements (the per-phase timing of one warmup step on pipeline
meshes).  ``--dump-outputs DIR`` writes what the last timed step
computed (loss, logits without the -inf vocab-padding columns, updated
parameters; seeded samples of the large ones) as ``DIR/<name>.npy``
after the timed region, every value finite.  With the option the step
keeps a reference to its last loss and logits (3.3 GB of bf16 logits for
GPT-2 124M at micro-batch 32, inside the captured graph's memory pool),
so such a run's memory layout differs from a plain run's; the timed
kernels are the same.  Multi-rank runs write ``<name>.rank<r>.npy`` per
rank.  Weights and data are seeded, so the same arguments give the same
inputs on every run.
"""

from __future__ import annotations

import argparse
import datetime
import json
import os
import time

# hipBLASLt algorithm selection via PyTorch TunableOp (+6% on the GPT-2
# step).  Tuning runs during the UNTIMED warmup steps; the result CSV is
# written explicitly after warmup (this build never writes it at exit)
# and committed under profiles/, so later runs load it and skip tuning.
# one shared CSV for every rank (local GEMM shapes are identical per
# rank on these meshes); only rank 0 writes
_TUNABLE_CSV = os.path.join(
    os.path.dirname(os.path.abspath(__file__)), "profiles",
    "tunableop_gfx950_0.csv",
)
os.environ.setdefault("PYTORCH_TUNABLEOP_ENABLED", "1")
os.environ.setdefault(
    "PYTORCH_TUNABLEOP_TUNING", "0" if os.path.exists(_TUNABLE_CSV) else "1"
)
os.environ.setdefault("PYTORCH_TUNABLEOP_FILENAME", _TUNABLE_CSV)

import torch
import torch.distributed as dist


def _write_tunableop_csv(path: str) -> None:
    res = torch.cuda.tunable.get_results()
    if not res:
        return
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        for k, v in torch.cuda.tunable.get_validators():
            f.write(f"Validator,{k},{v}\n")
        for r in res:
            f.write(",".join(str(x) for x in r) + "\n")


def parse_args():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--model", choices=["gpt2", "vit"], default="gpt2")
    p.add_argument("--gpt2-size", choices=["base", "medium", "large", "xl"],
                   default="base", help="GPT-2 preset for --model gpt2")
    p.add_argument("--micro-batch", type=int, default=None)
    p.add_argument("--grad-acc", type=int, default=None)
    p.add_argument("--seq-len", type=int, default=1024)
    p.add_argument("--tiny", action="store_true", help="tiny model for CPU smoke runs")
    p.add_argument("--sequence-parallel", action="store_true",
                   help="Megatron-SP over the TP axis (GPT-2)")
    p.add_argument("--full", action="store_true",
                   help="also run the secondary measurements (per-phase "
                        "timing of one warmup step on pipeline meshes)")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="after the timed steps, write the last step's "
                        "outputs to DIR/<name>.npy (float32)")
    return p.parse_args()


def pick_mesh(n: int):
    if n == 8:
        return [2, 2, 2]
    return [n, 1, 1]


def build_gpt2(args, pg, device, dtype):
    from quintnet_amd.models import GPT2Config, GPT2Stage
    from quintnet_amd.parallel import (
        DataParallel,
        DistributedConfig,
        PipelineParallelWrapper,
    )

    sp = args.sequence_parallel and pg.tp_size > 1
    interleaved = (
        os.environ.get("QN_SCHEDULE", "").lower().startswith("interleav")
        and pg.pp_size > 1
    )
    if interleaved:
        assert not sp, "interleaved bench: sequence parallelism unsupported"
        return _build_gpt2_interleaved(args, pg, device, dtype)
    if args.tiny:
        cfg = GPT2Config(n_embd=64, n_layer=2, n_head=2, vocab_size=512,
                         n_positions=args.seq_len, dropout=0.0,
                         sequence_parallel=sp)
    else:
        # vocab_pad_to=128: 50257 -> 50304 logits width (128-aligned
        # rows), IDENTICAL math — pad columns masked to -inf, zero grad
        # (models/gpt2/config.py; ~1 ms/step, profiles/vocab_pad_ab.md).
        # pp meshes default to 0: their M=8192 vocab GEMMs are tuned in
        # the CSV at 50257 but not at 50304 (tuning budget), and an
        # untuned library algo can cost more than alignment saves.
        pad_default = "128" if pg.pp_size == 1 else "0"
        cfg = GPT2Config.from_name(args.gpt2_size, dropout=0.0,
                                   n_positions=max(1024, args.seq_len),
                                   sequence_parallel=sp,
                                   vocab_pad_to=int(os.environ.get("QN_VOCAB_PAD", pad_default)),
                                   # QN_ACT_CKPT=1: recompute blocks in backward
                                   # (memory for ~1.33x fwd FLOPs — lets the
                                   # larger presets raise micro-batch)
                                   activation_checkpointing=os.environ.get("QN_ACT_CKPT") == "1")
    tp_group = pg.get_group("tp") if pg.tp_size > 1 else None
    stage = GPT2Stage(
        cfg,
        pp_rank=pg.pp_rank,
        pp_size=pg.pp_size,
        tp_group=tp_group,
        tied_group=pg.get_tied_embedding_group(),
        device=device,
        dtype=dtype,
    )
    # under SP the inter-stage activation is a sequence SHARD
    args.pipe_seq = args.seq_len // pg.tp_size if sp else args.seq_len
    pipe_seq = args.pipe_seq
    stage.seq_len = pipe_seq
    stage.hidden_dim = cfg.n_embd
    model = stage
    if pg.pp_size > 1:
        model = PipelineParallelWrapper(stage_module=stage, pp_rank=pg.pp_rank,
                                        pp_group=pg.get_group("pp"), pp_size=pg.pp_size,
                                        device=device)
        model.seq_len, model.hidden_dim = pipe_seq, cfg.n_embd
    if pg.dp_size > 1:
        model = DataParallel(model, DistributedConfig(
            pg.dp_rank, pg.dp_size, pg.get_group("dp")))
    return model, cfg


def _build_gpt2_interleaved(args, pg, device, dtype):
    """QN_SCHEDULE=interleaved: virtual-pipeline GPT-2 (2 chunks/rank by
    default, QN_VPP_CHUNKS to change)."""
    from quintnet_amd.models import GPT2Config, GPT2ForInterleaving
    from quintnet_amd.parallel import (
        DataParallel,
        DistributedConfig,
        InterleavedPipelineWrapper,
    )

    if args.tiny:
        cfg = GPT2Config(n_embd=64, n_layer=4, n_head=2, vocab_size=512,
                         n_positions=args.seq_len, dropout=0.0)
    else:
        # interleaved runs only at pp>1 — same tuned-shape rationale
        cfg = GPT2Config(dropout=0.0, n_positions=max(1024, args.seq_len),
                         vocab_pad_to=int(os.environ.get("QN_VOCAB_PAD", "0")))
    tp_group = pg.get_group("tp") if pg.tp_size > 1 else None
    full = GPT2ForInterleaving(cfg, tp_group=tp_group, device=device, dtype=dtype)
    chunks = int(os.environ.get("QN_VPP_CHUNKS", "2"))
    model = InterleavedPipelineWrapper(
        full, pp_rank=pg.pp_rank, pp_group=pg.get_group("pp"),
        pp_size=pg.pp_size, num_chunks=chunks, device=device,
        tied_group=pg.get_tied_embedding_group()
        if pg.pp_rank in (0, pg.pp_size - 1) else None,
    )
    args.pipe_seq = args.seq_len
    model.seq_len, model.hidden_dim = args.seq_len, cfg.n_embd
    if pg.dp_size > 1:
        model = DataParallel(model, DistributedConfig(
            pg.dp_rank, pg.dp_size, pg.get_group("dp")))
    return model, cfg


def build_vit(args, pg, device, dtype):
    from quintnet_amd.models import Model
    from quintnet_amd.parallel import (
        DataParallel,
        DistributedConfig,
        PipelineParallelWrapper,
        apply_tensor_parallel,
    )

    model = Model(hidden_dim=64, n_heads=4, depth=8)
    model = model.to(device=device, dtype=dtype)
    if pg.tp_size > 1:
        apply_tensor_parallel(model, tp_size=pg.tp_size, tp_rank=pg.tp_rank,
                              tp_group=pg.get_group("tp"), device=device)
    if pg.pp_size > 1:
        model = PipelineParallelWrapper(model=model, pp_rank=pg.pp_rank,
                                        pp_group=pg.get_group("pp"), pp_size=pg.pp_size,
                                        device=device)
    if pg.dp_size > 1:
        model = DataParallel(model, DistributedConfig(
            pg.dp_rank, pg.dp_size, pg.get_group("dp")))
    return model, None


# --dump-outputs budget: every array is float32; the total stays far
# below 64 MB (logits 4 MB + <= 64 KB per parameter tensor)
_DUMP_LOGITS = 1 << 20
_DUMP_PER_PARAM = 1 << 14


def _sample(t, limit, seed, width=None):
    """``t`` as a flat float32 numpy array; tensors above ``limit``
    elements are reduced to a fixed (seeded, sorted) sample of indices.
    ``width`` keeps only the first ``width`` entries of the last dim."""
    t = t.detach()
    if width is not None and width < t.shape[-1]:
        t = t[..., :width]
    n = t.numel()
    if n > limit:
        g = torch.Generator(device="cpu").manual_seed(seed)
        idx = torch.randint(0, n, (limit,), generator=g).sort().values
        idx = idx.to(t.device)
        w = t.shape[-1]
        # row/column gather: no contiguous copy of a sliced tensor
        t = t.reshape(-1, w)[idx // w, idx % w]
    return t.reshape(-1).float().cpu().numpy()


def dump_outputs(out_dir, model, last, rank, world_size):
    """Write what the last timed step produced: its loss and logits
    (where this rank has them) and the parameters it left behind.
    The vocab-padding logits columns (-inf by construction, never read by
    a caller) are left out: ``last["logits_pad"]`` trailing columns."""
    import numpy as np

    os.makedirs(out_dir, exist_ok=True)
    suffix = f".rank{rank}" if world_size > 1 else ""
    arrays = {}
    if last.get("loss") is not None:
        loss = last["loss"]
        if torch.is_tensor(loss):
            loss = loss.detach().float().cpu().item()
        arrays["loss"] = np.asarray([loss], dtype=np.float32)
    if last.get("logits") is not None:
        logits = last["logits"]
        width = logits.shape[-1] - last.get("logits_pad", 0)
        arrays["logits"] = _sample(logits, _DUMP_LOGITS, 4321, width)
    params = [_sample(p, _DUMP_PER_PARAM, 5000 + i)
              for i, p in enumerate(model.parameters())]
    if params:
        arrays["params"] = np.concatenate(params)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, f"{name}{suffix}.npy"),
                a.astype(np.float32, copy=False))


class _ListLoader:
    """PipelineDataLoader-compatible infinite loader over device-resident batches."""

    def __init__(self, batches, grad_acc_steps):
        self.batches = batches
        self.grad_acc_steps = grad_acc_steps
        self.i = 0

    def __len__(self):
        return 1 << 30

    def __iter__(self):
        return self

    def __next__(self):
        b = self.batches[self.i % len(self.batches)]
        self.i += 1
        return b


def main():
    args = parse_args()
    n = args.gpus
    use_cuda = torch.cuda.is_available()
    dtype = torch.bfloat16 if use_cuda else torch.float32
    if args.tiny and not use_cuda:
        dtype = torch.float32

    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != n and world > 1:
        n = world
    backend = "nccl" if use_cuda else "gloo"
    if use_cuda:
        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", 0)))
    if n > 1 and not dist.is_initialized():
        dist.init_process_group(backend=backend,
                                timeout=datetime.timedelta(seconds=600))

    from quintnet_amd import init_process_groups
    from quintnet_amd.optim import ZeroRedundancyAdamW
    from quintnet_amd.parallel import PipelineTrainer

    mesh = pick_mesh(n)
    pg = init_process_groups("cuda" if use_cuda else "cpu", mesh, ["dp", "tp", "pp"])
    device = pg.device
    rank = pg.rank
    # seeded weights (the data generators below are seeded too): the same
    # arguments give the same inputs on every run
    torch.manual_seed(1234 + rank)

    if args.model == "gpt2":
        # pp>1 wants >=4 micro-batches for 1F1B overlap; pp=1 prefers
        # bigger GEMMs (same 32 seqs/replica/step either way; micro 32
        # measured 47.7 vs micro16's 53.9 ms on one box, r2)
        pp = 2 if n == 8 else 1
        micro_b = args.micro_batch or (8 if pp > 1 else 32)
        grad_acc = args.grad_acc or (4 if pp > 1 else 1)
        model, cfg = build_gpt2(args, pg, device, dtype)
        vocab = cfg.vocab_size
        g = torch.Generator(device="cpu").manual_seed(1234 + pg.dp_rank)
        batches = []
        for _ in range(4):
            ids = torch.randint(0, vocab, (micro_b, args.seq_len), generator=g).to(device)
            batches.append({"input_ids": ids, "labels": ids.clone()})
        task = "clm"
        seq, hidden = args.seq_len, cfg.n_embd
        pipe_shape_seq = getattr(args, "pipe_seq", seq)
        sizes = {"base": "gpt2-124M", "medium": "gpt2-355M",
                 "large": "gpt2-774M", "xl": "gpt2-1.6B"}
        model_name = sizes[args.gpt2_size] if not args.tiny else "gpt2-tiny"
    else:
        micro_b = args.micro_batch or 16
        grad_acc = args.grad_acc or 4
        model, _ = build_vit(args, pg, device, dtype)
        g = torch.Generator(device="cpu").manual_seed(1234 + pg.dp_rank)
        batches = []
        for _ in range(4):
            x = torch.randn(micro_b, 1, 28, 28, generator=g).to(device=device, dtype=dtype)
            y = torch.randint(0, 10, (micro_b,), generator=g).to(device)
            batches.append({"images": x, "labels": y})
        task = "classification"
        seq, hidden = 50, 64
        model_name = "vit-mnist"

    loader = _ListLoader(batches, grad_acc)
    from quintnet_amd.ops import causal_lm_loss
    from quintnet_amd.parallel import DataParallel

    zero_kw = dict(lr=1e-4, weight_decay=0.01, max_grad_norm=1.0,
                   dp_group=pg.get_group("dp") if pg.dp_size > 1 else None,
                   tp_group=pg.get_group("tp") if pg.tp_size > 1 else None,
                   pp_group=pg.get_group("pp") if pg.pp_size > 1 else None)
    if isinstance(model, DataParallel):
        optimizer = ZeroRedundancyAdamW.from_ddp(model, **zero_kw)
    else:
        optimizer = ZeroRedundancyAdamW(model.parameters(), **zero_kw)

    criterion = torch.nn.CrossEntropyLoss(ignore_index=-100)
    # --dump-outputs: the step keeps a reference to its last loss/logits
    last = {}
    keep = args.dump_outputs is not None
    if args.model == "gpt2" and pg.tp_rank == pg.tp_size - 1:
        # the padding columns sit at the end of the (last shard's) logits
        last["logits_pad"] = cfg.padded_vocab_size - cfg.vocab_size

    if pg.pp_size > 1:
        groups = pg.get_all_groups()
        ptrainer = PipelineTrainer(
            model=model, optimizer=optimizer, criterion=criterion,
            pp_rank=pg.pp_rank, pp_size=pg.pp_size,
            pp_group=pg.get_group("pp"), pp_group_ranks=pg.get_group_ranks("pp"),
            schedule=os.environ.get("QN_SCHEDULE", "1f1b"),
            task_type=task, max_grad_norm=1.0,
            pp_fwd_group=groups.get("pp_fwd"), pp_bwd_group=groups.get("pp_bwd"),
            # QN_DEFER_WGRADS=1: zero-bubble dW deferral (A/B on pp meshes)
            defer_wgrads=os.environ.get("QN_DEFER_WGRADS") == "1",
        )
        shapes = (micro_b, pipe_shape_seq if task == "clm" else seq, hidden)

        def step():
            metrics = ptrainer.train_step(loader, shapes, device, dtype)
            if keep and isinstance(metrics, dict):
                last["loss"] = metrics.get("loss")

    else:
        is_ddp = isinstance(model, DataParallel)

        def step():
            if is_ddp:
                model.require_backward_grad_sync = False
            for i in range(grad_acc):
                b = next(loader)
                if is_ddp and i == grad_acc - 1:
                    model.require_backward_grad_sync = True
                if task == "clm":
                    logits = model(b["input_ids"])
                    loss = causal_lm_loss(logits, b["labels"], -100)
                else:
                    logits = model(b["images"])
                    loss = criterion(logits, b["labels"])
                (loss / grad_acc).backward()
                if keep:
                    last["loss"], last["logits"] = loss.detach(), logits.detach()
            if is_ddp:
                model.finalize_gradients()
            optimizer.step()
            if is_ddp:
                model.zero_grad()
            else:
                optimizer.zero_grad()

        # hipGraph capture of the whole optimizer step (single-GPU path):
        # the launch-bound inner loop replays as one graph; fresh data is
        # copied into the captured static input buffers before each replay.
        # ViT (launch-bound): 3.3x.  GPT-2: the round-1 HSA aperture fault
        # no longer reproduces (tools/graph_bisect.py r2: full-size
        # fwd+bwd+ZeRO captures clean) and capture is worth ~2 ms/step
        # (55.98 vs 57.9 ms) — on by default, QN_NO_GRAPHS=1 to disable.
        want_graphs = os.environ.get("QN_GRAPHS", "1") != "0"
        if (use_cuda and pg.world_size == 1 and want_graphs
                and os.environ.get("QN_NO_GRAPHS") != "1"):
            try:
                from quintnet_amd.utils.graphs import CapturedStep

                static_batches = [
                    {k: v.clone() for k, v in batches[i % len(batches)].items()}
                    for i in range(grad_acc)
                ]
                loader.batches = static_batches

                def reset_and_step():
                    loader.i = 0
                    step()

                captured = CapturedStep(reset_and_step, static_batches)
                state = {"i": 0}

                def graph_step():
                    feed = [
                        batches[(state["i"] + j) % len(batches)] for j in range(grad_acc)
                    ]
                    state["i"] += grad_acc
                    captured(feed)

                step = graph_step
                if rank == 0:
                    print("# hipGraph capture active", flush=True)
            except Exception as e:  # noqa: BLE001 — fall back to eager launches
                if rank == 0:
                    print(f"# hipGraph capture unavailable ({e!r}); eager path", flush=True)

    # hang watchdog (multi-rank runs): if any collective wedges, kill THIS
    # process with a stack dump instead of hanging the node until the
    # driver's own limit (default 600 s per beat; QN_WATCHDOG=0 disables)
    wd = None
    if pg.world_size > 1 and os.environ.get("QN_WATCHDOG", "1") != "0":
        from quintnet_amd.utils.watchdog import Watchdog

        wd = Watchdog(float(os.environ.get("QN_WATCHDOG_S", "600")),
                      kill_on_hang=True).start()

    def sync():
        if dist.is_initialized():
            dist.barrier()
        if use_cuda:
            torch.cuda.synchronize()

    # hardware ramp: a freshly-leased box runs its first ~2 s of kernels
    # at reduced effective clocks (measured: the FIRST bench on a box is
    # ~2.5-4 ms/step slower than an immediate re-run — profiles/ab_*.log).
    # Spin large GEMMs briefly so the driver's one-shot run measures
    # steady-state silicon, not the DVFS ramp.  This runs BEFORE the
    # contractual warmup steps and touches no benchmark state.
    if use_cuda:
        _a = torch.randn(8192, 8192, device=device, dtype=torch.bfloat16)
        _t0 = time.perf_counter()
        while time.perf_counter() - _t0 < 2.0:
            for _ in range(64):
                _a @ _a
            torch.cuda.synchronize()
        del _a

    phase_ms = None
    for wi in range(args.warmup):
        if (args.full and wi == args.warmup - 1 and pg.world_size > 1
                and pg.pp_size > 1):
            # overlap evidence: per-phase HIP-event times for ONE warmup
            # step (forward/backward/P2P comm/optimizer) — reported in
            # the JSON, never inside the timed region
            from quintnet_amd.utils.profiling import PhaseTimer

            pt = PhaseTimer()
            ptrainer.phase_timer = pt
            step()
            if use_cuda:
                torch.cuda.synchronize()
            phase_ms = {k: round(v, 2) for k, v in sorted(pt.summary().items())}
            ptrainer.phase_timer = None
        else:
            step()
        if wd:
            wd.beat()
    sync()
    if (use_cuda and os.environ.get("PYTORCH_TUNABLEOP_TUNING") == "1"
            and int(os.environ.get("RANK", "0")) == 0):
        try:
            # this build has no tunable.write_file() and never writes at
            # exit — serialize the results ourselves
            _write_tunableop_csv(_TUNABLE_CSV)
        except Exception:  # noqa: BLE001 — persistence is best-effort
            pass
    prof = None
    if os.environ.get("QN_TORCH_PROFILE") == "1" and use_cuda:
        # overlap-evidence timeline (chrome trace): NOT for timing runs —
        # profiling overhead lands inside the measured region.  Open the
        # trace at ui.perfetto.dev; comm kernels on their own stream
        # overlapping compute = the bucket/1F1B overlap proof.
        from torch.profiler import ProfilerActivity, profile

        prof = profile(
            activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA],
        )
        prof.__enter__()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
        if wd:
            wd.beat()
    sync()
    elapsed = time.perf_counter() - t0
    if prof is not None:
        prof.__exit__(None, None, None)
        os.makedirs("gpurun_out", exist_ok=True)
        tr = f"gpurun_out/trace_rank{os.environ.get('RANK', '0')}.json"
        prof.export_chrome_trace(tr)
        print(f"# torch-profiler trace -> {tr}", flush=True)
    if wd:
        wd.stop()
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, model, last, rank, pg.world_size)

    t = torch.tensor([elapsed], dtype=torch.float64)
    if dist.is_initialized():
        if use_cuda:
            t = t.to(device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    elapsed = float(t[0])

    samples_per_step = micro_b * grad_acc * pg.dp_size  # whole-job sequences/step
    value = samples_per_step * args.steps / elapsed
    ms_per_step = 1000.0 * elapsed / args.steps
    parallelism = f"dp{pg.dp_size}_tp{pg.tp_size}_pp{pg.pp_size}"
    result = {
        "metric": "samples/sec",
        "value": round(value, 3),
        "unit": "samples/s",
        "n_gpus": n,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(ms_per_step, 3),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "bf16" if dtype == torch.bfloat16 else "fp32",
        "data": "synthetic",
        "config": {
            "model": model_name,
            "global_batch": samples_per_step,
            "seq_len": seq if task == "clm" else None,
            "micro_batch": micro_b,
            "grad_acc": grad_acc,
            "parallelism": parallelism,
            "optimizer": "zero1-adamw",
            "tokens_per_sec": round(value * seq, 1) if task == "clm" else None,
            "warmup_phase_ms": phase_ms,
        },
    }
    if rank == 0:
        print(json.dumps(result), flush=True)
    if dist.is_initialized():
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
