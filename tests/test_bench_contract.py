"""bench.py driver contract: one JSON line on stdout with the agreed
keys (the round driver parses exactly this — a key rename or a stray
print on stdout breaks the BENCH/SCALE records)."""

import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_emits_contract_json():
    out = subprocess.run(
        [sys.executable, os.path.join(REPO, "bench.py"),
         "--tiny", "--gpus", "1", "--steps", "1", "--warmup", "0"],
        capture_output=True, text=True, timeout=600, cwd=REPO,
    )
    assert out.returncode == 0, out.stderr[-800:]
    payloads = []
    for ln in out.stdout.splitlines():
        ln = ln.strip()
        if ln.startswith("{"):
            payloads.append(json.loads(ln))
    assert len(payloads) == 1, out.stdout
    j = payloads[0]
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup",
                "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                "dtype", "data", "config"):
        assert key in j, key
    assert j["n_gpus"] == 1 and j["steps"] == 1 and j["warmup"] == 0
    assert j["higher_is_better"] is True and j["scaling"] == "weak"
    assert j["data"] == "synthetic"
    for ck in ("model", "global_batch", "seq_len", "parallelism"):
        assert ck in j["config"], ck
    assert j["value"] > 0 and j["ms_per_step"] > 0


def _bench_dump(out_dir, *extra):
    # hide any GPU: this test needs none and checks the CPU path
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    out = subprocess.run(
        [sys.executable, os.path.join(REPO, "bench.py"),
         "--tiny", "--seq-len", "64", "--gpus", "1", "--steps", "2",
         "--warmup", "1", "--dump-outputs", str(out_dir), *extra],
        capture_output=True, text=True, timeout=600, cwd=REPO, env=env,
    )
    assert out.returncode == 0, out.stderr[-800:]
    payloads = [json.loads(l) for l in out.stdout.splitlines()
                if l.strip().startswith("{")]
    assert len(payloads) == 1, out.stdout
    return payloads[0]


def test_bench_dump_outputs_and_full(tmp_path):
    """--dump-outputs writes the last step's outputs as float32 .npy
    (<= 64 MB in all); the same arguments give the same inputs, so on
    two runs agree bit for bit.  --full is accepted, keeps the result
    line's keys and does not change what is computed (what it gates, the
    per-phase timing on pipeline meshes, needs several ranks and is not
    exercised here)."""
    import numpy as np

    a = _bench_dump(tmp_path / "a")
    b = _bench_dump(tmp_path / "b", "--full")
    assert a["steps"] == b["steps"] == 2 and a["ms_per_step"] > 0
    assert set(a) == set(b) and set(a["config"]) == set(b["config"])
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["logits.npy", "loss.npy", "params.npy"]
    assert sorted(os.listdir(tmp_path / "b")) == names
    total = 0
    for n in names:
        x, y = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert x.dtype == np.float32 and x.size > 0, n
        assert np.isfinite(x).all(), n
        assert np.array_equal(x, y), n
        total += x.nbytes
    assert total <= 64 * 1024 * 1024
    # vocab 512 at random init: the loss is near ln(512)
    assert 5.0 < float(np.load(tmp_path / "a" / "loss.npy")[0]) < 8.0


_DUMP_UNIT = """
import sys, numpy as np, torch, bench
out = sys.argv[1]
model = torch.nn.Linear(4, 3)
logits = torch.arange(2 * 3 * 8, dtype=torch.float32).reshape(2, 3, 8)
logits[..., 6:] = float("-inf")  # two vocab-padding columns
last = {"loss": torch.tensor(1.5), "logits": logits, "logits_pad": 2}
bench.dump_outputs(out, model, last, rank=1, world_size=2)
got = np.load(out + "/logits.rank1.npy")
assert got.dtype == np.float32 and got.shape == (36,) and np.isfinite(got).all()
assert (got == logits[..., :6].reshape(-1).numpy()).all()
assert np.load(out + "/loss.rank1.npy").tolist() == [1.5]
assert np.load(out + "/params.rank1.npy").shape == (15,)
# above the limit: a fixed sample, the same on every call, padding excluded
a = bench._sample(logits, 10, 7, 6)
b = bench._sample(logits, 10, 7, 6)
assert a.shape == (10,) and (a == b).all() and np.isfinite(a).all()
print("ok")
"""


def test_dump_outputs_rank_names_and_padding(tmp_path):
    """dump_outputs: multi-rank runs write <name>.rank<r>.npy; the -inf
    vocab-padding columns of the logits are left out; the sample of a
    large tensor is fixed."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    out = subprocess.run(
        [sys.executable, "-c", _DUMP_UNIT, str(tmp_path)],
        capture_output=True, text=True, timeout=300, cwd=REPO, env=env,
    )
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stderr[-800:]
    assert sorted(os.listdir(tmp_path)) == [
        "logits.rank1.npy", "loss.rank1.npy", "params.rank1.npy"]


def test_bench_vit_contract():
    out = subprocess.run(
        [sys.executable, os.path.join(REPO, "bench.py"), "--model", "vit",
         "--tiny", "--gpus", "1", "--steps", "1", "--warmup", "0"],
        capture_output=True, text=True, timeout=600, cwd=REPO,
    )
    assert out.returncode == 0, out.stderr[-800:]
    payloads = [json.loads(l) for l in out.stdout.splitlines()
                if l.strip().startswith("{")]
    assert len(payloads) == 1
    assert payloads[0]["config"]["model"].startswith("vit")
