"""QN_ATTN_ORDER=balanced (default) against =linear and the fp32 oracle.

The launchers in csrc/attn.hip read QN_ATTN_ORDER once per process, so
each order runs in a child of its own, one after the other, on the same
seeded inputs; a child that does not exit 0 (a fault, an abort and a
timeout included) stops the module before the next one starts.  Each
child dumps out, lse2, dq, dk, dv per case; the parent compares

  * linear vs balanced: torch.equal on all five (a block's arithmetic does
    not depend on which block id runs it);
  * balanced vs fp32 SDPA at the tolerances of
    test_ops_gpu.py::test_flash_attention_vs_fp32.

Shapes: the smallest at which the block mapping can go wrong.

    (B, H, Tq, Tk, q_offset)   mask         what it exercises
    (1, 3, 128, 128, 0)        causal       one block per head, BH < 8
    (2, 3, 256, 256, 0)        causal, not  BH = 6 (no multiple of 8), nblk = 2
    (1, 8, 384, 384, 0)        causal       nblk = 3, BH = 8
    (3, 5, 1024, 1024, 0)      causal       nblk = 8 = XCD count, odd BH
    (2, 3, 128, 384, 256)      causal       context-parallel shard (Tq != Tk)

Run as a script (argument: output directory), this file is the child.
"""

import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {
    # name: (B, H, Tq, Tk, causal, q_offset, seed)
    "b1h3t128": (1, 3, 128, 128, True, 0, 11),
    "b2h3t256": (2, 3, 256, 256, True, 0, 12),
    "b2h3t256_noncausal": (2, 3, 256, 256, False, 0, 13),
    "b1h8t384": (1, 8, 384, 384, True, 0, 14),
    "b3h5t1024": (3, 5, 1024, 1024, True, 0, 15),
    "cp_tq128_tk384": (2, 3, 128, 384, True, 256, 16),
}
OUTPUTS = ("out", "lse2", "dq", "dk", "dv")
CHILD_TIMEOUT_S = 120

if __name__ != "__main__" and not torch.cuda.is_available():
    pytest.skip("needs MI355X", allow_module_level=True)


def _inputs(name):
    """Seeded q, k, v, dout of one case (generated on the CPU: the same
    bits in every process)."""
    B, H, tq, tk, _, _, seed = CASES[name]
    g = torch.Generator().manual_seed(seed)

    def rnd(t):
        return torch.randn(B, H, t, 64, generator=g).to(torch.bfloat16).cuda()

    return rnd(tq), rnd(tk), rnd(tk), rnd(tq)


def _child(outdir):
    from quintnet_amd import _C

    for name, (_, _, _, _, causal, q_offset, _) in CASES.items():
        q, k, v, dout = _inputs(name)
        out = torch.empty_like(q)
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        lse2 = _C.attn_fwd(q, k, v, out, 0.125, causal, q_offset)
        _C.attn_bwd(q, k, v, out, dout, lse2, dq, dk, dv, 0.125, causal, q_offset)
        torch.cuda.synchronize()
        torch.save({"out": out.cpu(), "lse2": lse2.cpu(), "dq": dq.cpu(),
                    "dk": dk.cpu(), "dv": dv.cpu()}, os.path.join(outdir, f"{name}.pt"))
    print("QN_ATTN_ORDER", os.environ.get("QN_ATTN_ORDER", "(unset)"), "done")


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    """{order: {case: {tensor name: tensor}}} from one child per order."""
    res = {}
    for order in ("linear", "balanced"):
        outdir = str(tmp_path_factory.mktemp(order))
        env = {k: v for k, v in os.environ.items() if not k.startswith("QN_ATTN_")}
        env["QN_ATTN_ORDER"] = order
        prev = env.get("PYTHONPATH")
        env["PYTHONPATH"] = f"{REPO}{os.pathsep}{prev}" if prev else REPO
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), outdir],
                               env=env, cwd=REPO, capture_output=True, text=True,
                               timeout=CHILD_TIMEOUT_S)
        except subprocess.TimeoutExpired:
            pytest.fail(f"child with QN_ATTN_ORDER={order} ran past {CHILD_TIMEOUT_S} s")
        # no further child after a failure of any kind
        assert r.returncode == 0, (order, r.returncode, r.stdout[-2000:], r.stderr[-2000:])
        res[order] = {name: torch.load(os.path.join(outdir, f"{name}.pt"))
                      for name in CASES}
    return res


@pytest.mark.parametrize("name", list(CASES))
def test_linear_and_balanced_bit_identical(dumps, name):
    for t in OUTPUTS:
        a, b = dumps["linear"][name][t], dumps["balanced"][name][t]
        assert a.shape == b.shape and torch.equal(a, b), (name, t)


@pytest.mark.parametrize("name", list(CASES))
def test_balanced_vs_fp32(dumps, name):
    _, _, tq, tk, causal, q_offset, _ = CASES[name]
    q, k, v, dout = _inputs(name)
    qf = q.float().requires_grad_(True)
    kf = k.float().requires_grad_(True)
    vf = v.float().requires_grad_(True)
    # query row i sits at global position i + q_offset: it sees keys <= that
    mask = (torch.ones(tq, tk, dtype=torch.bool, device=q.device).tril(q_offset)
            if causal else None)
    ref = torch.nn.functional.scaled_dot_product_attention(qf, kf, vf, attn_mask=mask)
    ref.backward(dout.float())
    got = dumps["balanced"][name]
    err = float((got["out"].cuda().float() - ref.detach()).abs().max())
    print(f"{name} out err {err:.3e}")
    assert err < 3e-2, (name, "out", err)
    for nm, rg in (("dq", qf.grad), ("dk", kf.grad), ("dv", vf.grad)):
        err = float((got[nm].cuda().float() - rg).abs().max())
        scale = max(float(rg.abs().max()), 1.0)
        print(f"{name} {nm} err {err:.3e} scale {scale:.3e}")
        assert err / scale < 4e-2, (name, nm, err, scale)


if __name__ == "__main__":
    _child(sys.argv[1])
