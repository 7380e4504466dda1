"""GPU: the fused decode-attention kernel (csrc/attn_decode.hip) against
fp32 row-by-row causal attention on the same bf16 inputs.

Shapes: B=2, H=3, D=64, Tmax=200 (ragged last 64-key split), scale 1/8,
q/k/v as views of one packed [B, T, 3*H*64] tensor.  Cache rows < past are
randn; every other row starts as NaN, so a read above the diagonal (or a
re-read of an appended row from the cache) shows as a non-finite output.
Tolerance: the flash-forward tolerance of tests/test_ops_gpu.py.
"""

import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    DEV = torch.device("cuda", 0)
else:
    pytest.skip("needs MI355X", allow_module_level=True)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, H, D, TMAX = 2, 3, 64, 200
TOL = dict(atol=2e-2, rtol=2e-2)
NAN = float("nan")


def _op():
    from quintnet_amd.ops import decode_attention, has_ext

    assert has_ext(), "HIP extension must be present on a GPU box"
    return decode_attention


def _heads(t, T):
    return t.view(B, T, H, D).permute(0, 2, 1, 3)


def _inputs(T, seed):
    """Packed qkv and its q/k/v [B,H,T,D] views (writes go through)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    qkv = torch.randn(B, T, 3 * H * D, generator=g).to(DEV, torch.bfloat16)
    hl = H * D
    q, k, v = (_heads(qkv[:, :, i * hl:(i + 1) * hl], T) for i in range(3))
    return qkv, q, k, v


def _caches(past, seed):
    g = torch.Generator(device="cpu").manual_seed(1000 + seed)
    kc = torch.randn(B, H, TMAX, D, generator=g).to(DEV, torch.bfloat16)
    vc = torch.randn(B, H, TMAX, D, generator=g).to(DEV, torch.bfloat16)
    kc[:, :, past:] = NAN
    vc[:, :, past:] = NAN
    return kc, vc


def _reference(q, k, v, kc0, vc0, past):
    """fp32 attention of row r over rows [0, past+r] of the cache with the
    new rows in place.  Returns (out [B,H,T,D] fp32, weights per row)."""
    T = q.shape[2]
    kf, vf = kc0.float().clone(), vc0.float().clone()
    kf[:, :, past:past + T] = k.float()
    vf[:, :, past:past + T] = v.float()
    out = torch.empty(B, H, T, D, device=DEV)
    weights = []
    for r in range(T):
        n = past + r + 1
        s = torch.einsum("bhd,bhjd->bhj", q[:, :, r].float(), kf[:, :, :n]) / 8.0
        p = torch.softmax(s, dim=-1)
        weights.append(p)
        out[:, :, r] = torch.einsum("bhj,bhjd->bhd", p, vf[:, :, :n])
    return out, weights


def _bits(t):
    return t.contiguous().view(torch.int16)


def _run(q, k, v, kc, vc, past):
    T = q.shape[2]
    buf = torch.empty(B, T, H * D, device=DEV, dtype=torch.bfloat16)
    p = torch.tensor(past, dtype=torch.long, device=DEV)
    out = _op()(q, k, v, kc, vc, p, out=_heads(buf, T))
    assert out.data_ptr() == buf.data_ptr()
    return out


def _check_caches(kc, vc, kc0, vc0, k, v, past):
    T = k.shape[2]
    assert torch.equal(_bits(kc[:, :, past:past + T]), _bits(k))
    assert torch.equal(_bits(vc[:, :, past:past + T]), _bits(v))
    keep = torch.ones(TMAX, dtype=torch.bool, device=DEV)
    keep[past:past + T] = False
    assert torch.equal(_bits(kc[:, :, keep]), _bits(kc0[:, :, keep]))
    assert torch.equal(_bits(vc[:, :, keep]), _bits(vc0[:, :, keep]))


@pytest.mark.parametrize("past", [0, 1, 63, 64, 65, 127, 128, 198, 199])
def test_boundary_sweep_single_row(past):
    _, q, k, v = _inputs(1, seed=past)
    kc, vc = _caches(past, seed=past)
    kc0, vc0 = kc.clone(), vc.clone()
    want, _ = _reference(q, k, v, kc0, vc0, past)
    out = _run(q, k, v, kc, vc, past)
    assert torch.isfinite(out.float()).all()
    err = (out.float() - want).abs().max().item()
    print(f"past={past} max abs err {err:.3e}")
    torch.testing.assert_close(out.float(), want, **TOL)
    if past == 0:  # one key, weight exactly 1
        assert torch.equal(_bits(out), _bits(v))
    _check_caches(kc, vc, kc0, vc0, k, v, past)


@pytest.mark.parametrize("j", [0, 63, 64, 127, 128, 198, 199])
def test_dropped_key_shows(j):
    """One key that holds > 90% of the softmax mass, value row +4: leaving
    it out moves the output by about 3."""
    past = 199
    _, q, k, v = _inputs(1, seed=50 + j)
    kc, vc = _caches(past, seed=50 + j)
    if j == past:  # the spike is the appended key itself
        k.copy_(1.5 * q)
        v.fill_(4.0)
    else:
        kc[:, :, j] = 1.5 * q[:, :, 0]
        vc[:, :, j] = 4.0
    kc0, vc0 = kc.clone(), vc.clone()
    want, weights = _reference(q, k, v, kc0, vc0, past)
    w = weights[0][:, :, j].min().item()
    print(f"spike j={j}: min reference weight {w:.4f}")
    assert w > 0.9, w
    out = _run(q, k, v, kc, vc, past)
    err = (out.float() - want).abs().max().item()
    print(f"spike j={j}: max abs err {err:.3e}")
    torch.testing.assert_close(out.float(), want, **TOL)


@pytest.mark.parametrize("past", [0, 62, 126, 192])
@pytest.mark.parametrize("T", [2, 5, 8])
def test_multi_row_causal(T, past):
    """Rows straddle split boundaries; past + T == Tmax at (8, 192).  The
    last new key is a spike against q row 0, which must not see it."""
    _, q, k, v = _inputs(T, seed=100 * T + past)
    k[:, :, T - 1] = 1.5 * q[:, :, 0]
    v[:, :, T - 1] = 4.0
    kc, vc = _caches(past, seed=100 * T + past)
    kc0, vc0 = kc.clone(), vc.clone()
    want, _ = _reference(q, k, v, kc0, vc0, past)
    out = _run(q, k, v, kc, vc, past)
    assert torch.isfinite(out.float()).all()
    for r in range(T):
        err = (out[:, :, r].float() - want[:, :, r]).abs().max().item()
        print(f"T={T} past={past} row {r}: max abs err {err:.3e}")
    # seeing the spike would pull row 0 towards +4 in every dim
    torch.testing.assert_close(out[:, :, 0].float(), want[:, :, 0], **TOL)
    torch.testing.assert_close(out.float(), want, **TOL)
    _check_caches(kc, vc, kc0, vc0, k, v, past)


def test_graph_replay_follows_device_position():
    op = _op()
    _, q, k, v = _inputs(1, seed=7)
    master_k, master_v = _caches(TMAX, seed=7)  # all rows randn

    def reset(kc, vc, p):
        kc.copy_(master_k)
        vc.copy_(master_v)
        kc[:, :, p:] = NAN
        vc[:, :, p:] = NAN

    kc, vc = master_k.clone(), master_v.clone()
    past = torch.zeros((), dtype=torch.long, device=DEV)
    buf = torch.empty(B, 1, H * D, device=DEV, dtype=torch.bfloat16)
    out = _heads(buf, 1)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            op(q, k, v, kc, vc, past, out=out)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        op(q, k, v, kc, vc, past, out=out)
    for p in (3, 64, 150):
        past.fill_(p)
        reset(kc, vc, p)
        buf.zero_()
        graph.replay()
        got, got_k, got_v = out.clone(), kc.clone(), vc.clone()
        ek, ev = master_k.clone(), master_v.clone()
        reset(ek, ev, p)
        want = _run(q, k, v, ek, ev, p)
        assert torch.isfinite(got.float()).all()
        assert torch.equal(_bits(got), _bits(want)), p
        assert torch.equal(_bits(got_k), _bits(ek)), p
        assert torch.equal(_bits(got_v), _bits(ev)), p


def test_deterministic():
    past, T = 150, 3
    _, q, k, v = _inputs(T, seed=9)
    outs = []
    for _ in range(2):
        kc, vc = _caches(past, seed=9)
        outs.append(_run(q, k, v, kc, vc, past).clone())
    assert torch.equal(_bits(outs[0]), _bits(outs[1]))


def test_decoder_fused_vs_composed_logits():
    from quintnet_amd.models import GPT2Config, GPT2Stage, StaticKVDecoder

    torch.manual_seed(0)
    cfg = GPT2Config(n_embd=128, n_head=2, n_layer=2, vocab_size=512,
                     n_positions=128, dropout=0.0)
    stage = GPT2Stage(cfg, device=DEV, dtype=torch.bfloat16).eval()
    ids = torch.randint(0, cfg.vocab_size, (2, 16), device=DEV)
    tok = torch.randint(0, cfg.vocab_size, (2, 1), device=DEV)
    logits = []
    with torch.no_grad():
        for fused in (True, False):
            dec = StaticKVDecoder(stage, batch=2, max_len=128,
                                  fused_attention=fused)
            assert dec.fused_attention is fused
            dec._forward_tokens(ids, dec.past)
            dec.past.fill_(16)
            logits.append(dec._forward_tokens(tok, dec.past).float())
    assert torch.isfinite(logits[0]).all()
    err = (logits[0] - logits[1]).abs().max().item()
    print(f"decoder logits: max abs diff {err:.3e}")
    torch.testing.assert_close(logits[0], logits[1], **TOL)
    assert StaticKVDecoder(stage, batch=2, max_len=128).fused_attention is True


def test_decode_kernels_spill_free():
    so = [f for f in os.listdir(os.path.join(REPO, "quintnet_amd"))
          if f.startswith("_C") and f.endswith(".so")]
    if not so:
        pytest.skip("extension not built")
    out = subprocess.run(
        [sys.executable, os.path.join(REPO, "tools", "dump_kernel_resources.py"),
         "attn_decode"],
        capture_output=True, text=True, timeout=300, cwd=REPO,
    )
    assert out.returncode == 0, out.stderr[-500:]
    rows = {}
    for ln in out.stdout.splitlines()[1:]:
        parts = ln.rsplit(None, 6)
        if len(parts) == 7:
            rows[parts[0].strip()] = int(parts[4])
    for frag in ("attn_decode_split_kernel<1>", "attn_decode_split_kernel<8>",
                 "attn_decode_combine_kernel"):
        match = [s for name, s in rows.items() if frag in name]
        assert match, (frag, sorted(rows))
        assert match[0] == 0, (frag, rows)
    assert all(s == 0 for s in rows.values()), rows
