"""Every flash-attention kernel instantiation vs the fp32 SDPA oracle.

The launchers in csrc/attn.hip read their knobs (QN_ATTN_FWD_OCC,
QN_ATTN_KLDS, QN_ATTN_DQ_OCC, QN_ATTN_DKV_OCC) once per process, so the
non-default kernels can only be reached from a fresh process: the test
starts one child per knob setting, strictly one after another, and stops
at the first child that does not exit 0 (a fault, an abort and a timeout
included).  The four settings cover all nine fwd/dq/dkv instantiations:

    setting                                   fwd         dq          dkv
    defaults                                  <3, true>   <3, true>   <2, true>
    FWD_OCC=4 KLDS=0 DQ_OCC=4 DKV_OCC=3       <4, false>  <4, false>  <3, false>
    FWD_OCC=4 DQ_OCC=2                        <4, true>   <2, true>   <2, true>
    KLDS=0                                    <3, false>  <3, true>   <2, true>

Run as a script, this file is the child: it checks out, dq, dk and dv at
the tolerances of test_ops_gpu.py::test_flash_attention_vs_fp32.
"""

import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = ("QN_ATTN_FWD_OCC", "QN_ATTN_KLDS", "QN_ATTN_DQ_OCC", "QN_ATTN_DKV_OCC")
SETTINGS = [
    {},
    {"QN_ATTN_FWD_OCC": "4", "QN_ATTN_KLDS": "0", "QN_ATTN_DQ_OCC": "4",
     "QN_ATTN_DKV_OCC": "3"},
    {"QN_ATTN_FWD_OCC": "4", "QN_ATTN_DQ_OCC": "2"},
    {"QN_ATTN_KLDS": "0"},
]
CHILD_TIMEOUT_S = 120

if __name__ != "__main__" and not torch.cuda.is_available():
    pytest.skip("needs MI355X", allow_module_level=True)


def _check(tq, tk, causal, q_offset, seed):
    """One shape, B=1 H=2 D=64 bf16, through FlashAttentionFunction."""
    from quintnet_amd.ops.attention import FlashAttentionFunction, _flash_ok

    torch.manual_seed(seed)
    dev = torch.device("cuda", 0)
    q = torch.randn(1, 2, tq, 64, device=dev, dtype=torch.bfloat16, requires_grad=True)
    k = torch.randn(1, 2, tk, 64, device=dev, dtype=torch.bfloat16, requires_grad=True)
    v = torch.randn(1, 2, tk, 64, device=dev, dtype=torch.bfloat16, requires_grad=True)
    assert _flash_ok(q)
    out = FlashAttentionFunction.apply(q, k, v, causal, q_offset)
    qf = q.detach().float().requires_grad_(True)
    kf = k.detach().float().requires_grad_(True)
    vf = v.detach().float().requires_grad_(True)
    # query row i sits at global position i + q_offset: it sees keys <= that
    mask = torch.ones(tq, tk, dtype=torch.bool, device=dev).tril(q_offset) if causal else None
    ref = torch.nn.functional.scaled_dot_product_attention(qf, kf, vf, attn_mask=mask)
    tag = f"Tq={tq} Tk={tk} causal={causal} q_offset={q_offset}"
    err = float((out.float() - ref).abs().max())
    print(f"{tag} out err {err:.3e}")
    assert err < 3e-2, (tag, "out", err)

    dout = torch.randn_like(out)
    out.backward(dout)
    ref.backward(dout.float())
    for g, rg, nm in ((q.grad, qf.grad, "dq"), (k.grad, kf.grad, "dk"), (v.grad, vf.grad, "dv")):
        err = float((g.float() - rg).abs().max())
        scale = max(float(rg.abs().max()), 1.0)
        print(f"{tag} {nm} err {err:.3e} scale {scale:.3e}")
        assert err / scale < 4e-2, (tag, nm, err, scale)


def _child():
    # T=256 is two 128-row blocks: the least that meets, in the q-major
    # (fwd, dq) and the key-major (dkv) loops, a skipped, a diagonal and a
    # full tile, and a tile whose prefetch two tiles ahead is not taken
    _check(256, 256, True, 0, seed=7)
    _check(256, 256, False, 0, seed=8)
    # rectangular, shifted diagonal (a context-parallel rank's shard)
    _check(128, 384, True, 256, seed=3)
    torch.cuda.synchronize()


def test_every_attention_instantiation_vs_fp32():
    for knobs in SETTINGS:
        env = {k: v for k, v in os.environ.items() if k not in KNOBS}
        env.update(knobs)
        prev = env.get("PYTHONPATH")
        env["PYTHONPATH"] = f"{REPO}{os.pathsep}{prev}" if prev else REPO
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env,
                               cwd=REPO, capture_output=True, text=True,
                               timeout=CHILD_TIMEOUT_S)
        except subprocess.TimeoutExpired:
            pytest.fail(f"child with {knobs} ran past {CHILD_TIMEOUT_S} s")
        print(f"--- {knobs or 'defaults'} ---\n{r.stdout}")
        # no further child after a failure of any kind
        assert r.returncode == 0, (knobs, r.returncode, r.stdout[-2000:], r.stderr[-2000:])


if __name__ == "__main__":
    _child()
