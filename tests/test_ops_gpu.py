"""GPU numerics: each hand-written gfx950 kernel vs a plain PyTorch fp32
reference of the same op (the SURVEY.md §4 oracle pattern)."""

import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    DEV = torch.device("cuda", 0)
else:
    pytest.skip("needs MI355X", allow_module_level=True)


def _ext():
    from quintnet_amd.ops import ext, has_ext

    assert has_ext(), "HIP extension must be present on a GPU box"
    return ext()


def test_ext_loaded():
    assert _ext().gfx == "gfx950"


@pytest.mark.parametrize("m,n,k", [(128, 128, 64), (256, 384, 128), (400, 50257 % 512 + 384, 72), (130, 100, 64), (8192 // 16, 768, 384)])
def test_gemm_nt_vs_fp32(m, n, k):
    torch.manual_seed(0)
    a = torch.randn(m, k, device=DEV, dtype=torch.bfloat16)
    b = torch.randn(n, k, device=DEV, dtype=torch.bfloat16)
    bias = torch.randn(n, device=DEV, dtype=torch.bfloat16)
    out = _ext().gemm_nt(a, b, bias, 0)[0]
    ref = (a.float() @ b.float().t() + bias.float())
    err = (out.float() - ref).abs().max() / max(float(ref.abs().max()), 1.0)
    assert err < 2e-2, err  # bf16 inputs, fp32 accum
    assert torch.isfinite(out.float()).all()


def test_gemm_nt_gelu_epilogue():
    torch.manual_seed(1)
    a = torch.randn(192, 128, device=DEV, dtype=torch.bfloat16)
    b = torch.randn(96, 128, device=DEV, dtype=torch.bfloat16)
    bias = torch.randn(96, device=DEV, dtype=torch.bfloat16)
    out, pre = _ext().gemm_nt(a, b, bias, 1)
    ref_pre = a.float() @ b.float().t() + bias.float()
    ref = torch.nn.functional.gelu(ref_pre, approximate="tanh")
    assert (pre.float() - ref_pre).abs().max() / float(ref_pre.abs().max()) < 2e-2
    scale = max(float(ref.abs().max()), 1.0)
    assert (out.float() - ref).abs().max() / scale < 2e-2


@pytest.mark.parametrize("rows,h", [(400, 64), (1024, 768), (77, 3072), (65, 100)])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
def test_layernorm_fwd_bwd(rows, h, dt):
    torch.manual_seed(2)
    x = torch.randn(rows, h, device=DEV, dtype=dt)
    w = torch.randn(h, device=DEV, dtype=dt)
    b = torch.randn(h, device=DEV, dtype=dt)
    y, mean, rstd = _ext().layernorm_fwd(x, w, b, 1e-5, None)
    ref = torch.nn.functional.layer_norm(x.float(), (h,), w.float(), b.float(), 1e-5)
    tol = 2e-2 if dt == torch.bfloat16 else 1e-5
    assert (y.float() - ref).abs().max() < tol * max(float(ref.abs().max()), 1.0)

    dy = torch.randn(rows, h, device=DEV, dtype=dt)
    dx, dw, db = _ext().layernorm_bwd(dy, x, w, mean, rstd, None)
    xf = x.float().requires_grad_(True)
    wf = w.float().requires_grad_(True)
    bf = b.float().requires_grad_(True)
    rr = torch.nn.functional.layer_norm(xf, (h,), wf, bf, 1e-5)
    gx, gw, gb = torch.autograd.grad(rr, (xf, wf, bf), dy.float())
    s = max(float(gx.abs().max()), 1.0)
    dx_tol = 3e-2 * s if dt == torch.bfloat16 else 1e-4 * s
    assert (dx.float() - gx).abs().max() < dx_tol
    assert (dw.float() - gw).abs().max() / max(float(gw.abs().max()), 1.0) < 3e-2
    assert (db.float() - gb).abs().max() / max(float(gb.abs().max()), 1.0) < 3e-2


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
def test_softmax_fwd_bwd(causal, dt):
    torch.manual_seed(3)
    B, H, T, S = 2, 3, 64, 64
    s = torch.randn(B, H, T, S, device=DEV, dtype=dt)
    scale = 1.0 / math.sqrt(16)
    p = _ext().softmax_fwd(s, scale, causal)
    sf = s.float() * scale
    if causal:
        mask = torch.ones(T, S, dtype=torch.bool, device=DEV).tril()
        sf = sf.masked_fill(~mask, float("-inf"))
    ref = torch.softmax(sf, dim=-1)
    tol = 1e-2 if dt == torch.bfloat16 else 1e-5
    assert (p.float() - ref).abs().max() < tol
    if causal:
        assert float(p.float()[..., 0, 1:].abs().max()) == 0.0

    dp = torch.randn_like(s)
    ds = _ext().softmax_bwd(p, dp, scale)
    row = (ref * dp.float()).sum(-1, keepdim=True)
    ref_ds = scale * ref * (dp.float() - row)
    assert (ds.float() - ref_ds).abs().max() < (3e-2 if dt == torch.bfloat16 else 1e-5)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
def test_cross_entropy_fwd_bwd(dt):
    torch.manual_seed(4)
    N, V = 512, 50257
    logits = torch.randn(N, V, device=DEV, dtype=dt)
    tgt = torch.randint(0, V, (N,), device=DEV)
    tgt[::5] = -100
    loss_sum, n_valid, lse = _ext().cross_entropy_fwd(logits, tgt, -100)
    loss = loss_sum / n_valid.clamp_min(1).float()
    ref = torch.nn.functional.cross_entropy(logits.float(), tgt, ignore_index=-100)
    tol = 2e-2 if dt == torch.bfloat16 else 1e-4
    assert abs(float(loss) - float(ref)) < tol, (float(loss), float(ref))

    dl = _ext().cross_entropy_bwd(logits, tgt, lse, n_valid, -100, None)
    lf = logits.float().requires_grad_(True)
    rr = torch.nn.functional.cross_entropy(lf, tgt, ignore_index=-100)
    (g,) = torch.autograd.grad(rr, lf)
    assert (dl.float() - g).abs().max() < 1e-3


def test_adamw_step_vs_torch():
    torch.manual_seed(5)
    n = 10007
    master = torch.randn(n, device=DEV, dtype=torch.float32)
    param = master.to(torch.bfloat16)
    grad = torch.randn(n, device=DEV, dtype=torch.bfloat16)
    m = torch.zeros(n, device=DEV)
    v = torch.zeros(n, device=DEV)

    ref = master.clone().requires_grad_(True)
    opt = torch.optim.AdamW([ref], lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
    for step in range(1, 4):
        _ext().adamw_step(param, master, grad, m, v, step, 1e-2, 0.9, 0.999, 1e-8, 0.01, None)
        ref.grad = grad.float()
        opt.step()
    assert (master - ref.detach()).abs().max() < 1e-4
    assert (param.float() - master).abs().max() < 0.02  # bf16 rounding


def test_multi_tensor_sumsq():
    xs = [torch.randn(1000, device=DEV), torch.randn(37, device=DEV, dtype=torch.bfloat16)]
    out = _ext().multi_tensor_sumsq(xs)
    ref = sum(float(x.float().pow(2).sum()) for x in xs)
    assert abs(float(out) - ref) / ref < 1e-2


def test_fused_attention_op_vs_sdpa():
    from quintnet_amd.ops import attention

    torch.manual_seed(6)
    q = torch.randn(2, 4, 128, 64, device=DEV, dtype=torch.bfloat16, requires_grad=True)
    k = torch.randn(2, 4, 128, 64, device=DEV, dtype=torch.bfloat16, requires_grad=True)
    v = torch.randn(2, 4, 128, 64, device=DEV, dtype=torch.bfloat16, requires_grad=True)
    out = attention(q, k, v, causal=True)
    ref = torch.nn.functional.scaled_dot_product_attention(
        q.float(), k.float(), v.float(), is_causal=True
    )
    assert (out.float() - ref).abs().max() < 3e-2
    out.sum().backward()
    assert torch.isfinite(q.grad.float()).all()


def test_model_linear_uses_native_gemm():
    """The TP-linear path must run the hand-written GEMM on GPU."""
    from quintnet_amd.ops import linear

    x = torch.randn(256, 128, device=DEV, dtype=torch.bfloat16, requires_grad=True)
    w = torch.randn(256, 128, device=DEV, dtype=torch.bfloat16, requires_grad=True)
    b = torch.randn(256, device=DEV, dtype=torch.bfloat16, requires_grad=True)
    y = linear(x, w, b, activation="gelu")
    ref = torch.nn.functional.gelu(
        torch.nn.functional.linear(x.float(), w.float(), b.float()), approximate="tanh"
    )
    assert (y.float() - ref).abs().max() / max(float(ref.abs().max()), 1.0) < 3e-2
    y.sum().backward()
    for t in (x, w, b):
        assert torch.isfinite(t.grad.float()).all()


@pytest.mark.parametrize("causal", [True, False])
def test_flash_attention_vs_fp32(causal):
    """Fully-fused flash kernel vs fp32 SDPA (fwd + all three grads)."""
    from quintnet_amd.ops.attention import FlashAttentionFunction, _flash_ok

    torch.manual_seed(7)
    B, H, T, D = 2, 3, 256, 64
    q = torch.randn(B, H, T, D, device=DEV, dtype=torch.bfloat16, requires_grad=True)
    k = torch.randn(B, H, T, D, device=DEV, dtype=torch.bfloat16, requires_grad=True)
    v = torch.randn(B, H, T, D, device=DEV, dtype=torch.bfloat16, requires_grad=True)
    assert _flash_ok(q)
    out = FlashAttentionFunction.apply(q, k, v, causal)
    qf = q.detach().float().requires_grad_(True)
    kf = k.detach().float().requires_grad_(True)
    vf = v.detach().float().requires_grad_(True)
    ref = torch.nn.functional.scaled_dot_product_attention(qf, kf, vf, is_causal=causal)
    assert (out.float() - ref).abs().max() < 3e-2, (out.float() - ref).abs().max()

    dout = torch.randn_like(out)
    out.backward(dout)
    ref.backward(dout.float())
    for g, rg, nm in ((q.grad, qf.grad, "dq"), (k.grad, kf.grad, "dk"), (v.grad, vf.grad, "dv")):
        err = (g.float() - rg).abs().max()
        scale = max(float(rg.abs().max()), 1.0)
        assert err / scale < 4e-2, (nm, err, scale)


def test_flash_attention_qkv_packed():
    """Packed-QKV fused path == composed reference, incl. dqkv."""
    from quintnet_amd.ops import attention_qkv

    torch.manual_seed(8)
    B, T, Hh, D = 2, 128, 4, 64
    hl = Hh * D
    qkv = torch.randn(B, T, 3 * hl, device=DEV, dtype=torch.bfloat16, requires_grad=True)
    out = attention_qkv(qkv, Hh, causal=True)

    qkv2 = qkv.detach().float().requires_grad_(True)
    q, k, v = qkv2.split(hl, dim=-1)

    def heads(t):
        return t.view(B, T, Hh, D).transpose(1, 2)

    ref = torch.nn.functional.scaled_dot_product_attention(
        heads(q), heads(k), heads(v), is_causal=True
    ).transpose(1, 2).reshape(B, T, hl)
    assert (out.float() - ref).abs().max() < 3e-2

    dout = torch.randn_like(out)
    out.backward(dout)
    ref.backward(dout.float())
    err = (qkv.grad.float() - qkv2.grad).abs().max()
    scale = max(float(qkv2.grad.abs().max()), 1.0)
    assert err / scale < 4e-2, err


def test_flash_attention_long_seq():
    """T=1024 (the bench shape): finite + row-sum sanity vs SDPA."""
    from quintnet_amd.ops.attention import FlashAttentionFunction

    torch.manual_seed(9)
    q = torch.randn(1, 2, 1024, 64, device=DEV, dtype=torch.bfloat16)
    k = torch.randn(1, 2, 1024, 64, device=DEV, dtype=torch.bfloat16)
    v = torch.randn(1, 2, 1024, 64, device=DEV, dtype=torch.bfloat16)
    out = FlashAttentionFunction.apply(q, k, v, True)
    ref = torch.nn.functional.scaled_dot_product_attention(
        q.float(), k.float(), v.float(), is_causal=True
    )
    assert (out.float() - ref).abs().max() < 3e-2


def test_fused_dropout():
    from quintnet_amd.ops import fused_dropout

    x = torch.ones(100000, device=DEV, dtype=torch.bfloat16, requires_grad=True)
    y = fused_dropout(x, 0.3, training=True)
    kept = (y != 0).float().mean()
    assert abs(float(kept) - 0.7) < 0.02, float(kept)
    # kept values scaled by 1/(1-p)
    nz = y[y != 0].float()
    assert torch.allclose(nz, torch.full_like(nz, 1.0 / 0.7), atol=1e-2)
    y.sum().backward()
    g = x.grad.float()
    assert torch.allclose((g != 0).float().mean(), kept, atol=1e-3)
    # eval mode / p=0: identity
    assert fused_dropout(x, 0.3, training=False) is x


def test_layernorm_residual_fused():
    from quintnet_amd.ops import layer_norm_residual

    torch.manual_seed(11)
    x = torch.randn(64, 768, device=DEV, dtype=torch.bfloat16, requires_grad=True)
    r = torch.randn(64, 768, device=DEV, dtype=torch.bfloat16, requires_grad=True)
    w = torch.randn(768, device=DEV, dtype=torch.bfloat16, requires_grad=True)
    b = torch.randn(768, device=DEV, dtype=torch.bfloat16, requires_grad=True)
    y, s = layer_norm_residual(x, r, w, b, 1e-5)
    xf = x.detach().float().requires_grad_(True)
    rf = r.detach().float().requires_grad_(True)
    wf = w.detach().float().requires_grad_(True)
    bf = b.detach().float().requires_grad_(True)
    sf = xf + rf
    yf = torch.nn.functional.layer_norm(sf, (768,), wf, bf, 1e-5)
    assert (s.float() - sf).abs().max() < 2e-2
    assert (y.float() - yf).abs().max() < 3e-2
    dy = torch.randn_like(y)
    ds = torch.randn_like(s)
    (y * dy.detach() + s * ds.detach()).sum().backward()
    (yf * dy.detach().float() + sf * ds.detach().float()).sum().backward()
    for g, rg in ((x.grad, xf.grad), (r.grad, rf.grad)):
        assert (g.float() - rg).abs().max() / max(float(rg.abs().max()), 1.0) < 4e-2
    assert (w.grad.float() - wf.grad).abs().max() / max(float(wf.grad.abs().max()), 1.0) < 4e-2


def test_embedding_pair_fused():
    from quintnet_amd.ops import embedding_pair

    torch.manual_seed(12)
    V, P, H = 512, 64, 256
    wte = torch.randn(V, H, device=DEV, dtype=torch.bfloat16, requires_grad=True)
    wpe = torch.randn(P, H, device=DEV, dtype=torch.bfloat16, requires_grad=True)
    ids = torch.randint(0, V, (4, 32), device=DEV)
    out = embedding_pair(ids, wte, wpe)
    pos = torch.arange(32, device=DEV)
    ref = torch.nn.functional.embedding(ids, wte.float()) + torch.nn.functional.embedding(pos, wpe.float())
    assert (out.float() - ref).abs().max() < 2e-2
    dout = torch.randn_like(out)
    out.backward(dout)
    wtef = wte.detach().float().requires_grad_(True)
    wpef = wpe.detach().float().requires_grad_(True)
    (torch.nn.functional.embedding(ids, wtef) +
     torch.nn.functional.embedding(pos, wpef)).backward(dout.float())
    assert (wte.grad.float() - wtef.grad).abs().max() / max(float(wtef.grad.abs().max()), 1.0) < 3e-2
    assert (wpe.grad.float() - wpef.grad).abs().max() / max(float(wpef.grad.abs().max()), 1.0) < 3e-2


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
def test_embedding_bwd_heavy_duplicates(dt):
    """Atomic-free scatter-add: token runs inside one 16-position chunk,
    runs of ~40 that cross chunk borders and one padding-like token that
    fills about half the rows (a run over ~30 chunks); H=200 is no
    multiple of the 128-column tile; position table longer than the
    sequence; a vocab row that never occurs.  fp32 sums of <= ~600
    addends of |x| ~ 1: error << 1e-3; the bf16 result adds only its final
    rounding, at most 2^-8 relative."""
    torch.manual_seed(13)
    V, P, B, T, H = 40, 160, 8, 125, 200
    ids = torch.randint(0, V - 1, (B, T), device=DEV)  # token V-1 unused
    ids[torch.rand(B, T, device=DEV) < 0.5] = 3
    ids[0, :12] = torch.arange(20, 32, device=DEV)[:12]
    dout = torch.randn(B, T, H, device=DEV, dtype=dt)
    dwte, dwpe = _ext().embedding_pair_bwd(ids, dout, V, P)
    ref_te = torch.zeros(V, H, device=DEV, dtype=torch.float64).index_add_(
        0, ids.reshape(-1), dout.double().reshape(-1, H)).float()
    ref_pe = torch.zeros(P, H, device=DEV)
    ref_pe[:T] = dout.double().sum(0).float()
    rel = 2.0 ** -8 if dt == torch.bfloat16 else 0.0
    assert dwte.shape == (V, H) and dwpe.shape == (P, H)
    assert bool(((dwte.float() - ref_te).abs() <= rel * ref_te.abs() + 1e-3).all())
    assert bool(((dwpe.float() - ref_pe).abs() <= rel * ref_pe.abs() + 1e-3).all())
    assert float(dwte[V - 1].abs().max()) == 0.0
    assert float(dwpe[T:].abs().max()) == 0.0


def test_reductions_bit_reproducible():
    """The reductions that feed the weights and the loss (embedding
    scatter-add, LayerNorm dw/db, grad-norm sum of squares, CE loss sum)
    add in a fixed order: the same call twice gives the same bits."""
    torch.manual_seed(14)
    e = _ext()
    ids = torch.randint(0, 16, (8, 128), device=DEV)
    dout = torch.randn(8, 128, 768, device=DEV, dtype=torch.bfloat16)
    a, b = e.embedding_pair_bwd(ids, dout, 16, 128), e.embedding_pair_bwd(ids, dout, 16, 128)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])

    x = torch.randn(4096, 768, device=DEV, dtype=torch.bfloat16)
    w = torch.randn(768, device=DEV, dtype=torch.bfloat16)
    dy = torch.randn_like(x)
    mean = x.float().mean(-1)
    rstd = (x.float().var(-1, unbiased=False) + 1e-5).rsqrt()
    a, b = e.layernorm_bwd(dy, x, w, mean, rstd, None), e.layernorm_bwd(dy, x, w, mean, rstd, None)
    assert all(torch.equal(p, q) for p, q in zip(a, b))

    # 600k elements: past the 2048-block cap of the sum-of-squares grid
    xs = [torch.randn(600_000, device=DEV), torch.randn(1000, device=DEV, dtype=torch.bfloat16)]
    assert torch.equal(e.multi_tensor_sumsq(xs), e.multi_tensor_sumsq(xs))
    ref = sum(float(t.double().pow(2).sum()) for t in xs)
    assert abs(float(e.multi_tensor_sumsq(xs)) - ref) / ref < 1e-5

    logits = torch.randn(3000, 1000, device=DEV, dtype=torch.bfloat16)
    tgt = torch.randint(0, 1000, (3000,), device=DEV)
    tgt[::7] = -100
    a, b = e.cross_entropy_fwd(logits, tgt, -100), e.cross_entropy_fwd(logits, tgt, -100)
    assert torch.equal(a[0], b[0])


@pytest.mark.gpu
def test_flash_attention_q_offset_vs_reference():
    """Rectangular flash attention with a shifted causal diagonal (the CP
    path): HIP kernels vs the plain fp32 reference, forward + backward."""
    import math

    from quintnet_amd.ops.attention import FlashAttentionFunction

    torch.manual_seed(3)
    B, H, Tk, D = 2, 4, 512, 64
    cp = 4
    Tq = Tk // cp
    k = torch.randn(B, H, Tk, D, device="cuda", dtype=torch.bfloat16)
    v = torch.randn(B, H, Tk, D, device="cuda", dtype=torch.bfloat16)
    full_q = torch.randn(B, H, Tk, D, device="cuda", dtype=torch.bfloat16)
    scale = 1.0 / math.sqrt(D)
    for r in range(cp):
        qoff = r * Tq
        q = full_q[:, :, qoff : qoff + Tq].contiguous().requires_grad_(True)
        kk = k.clone().requires_grad_(True)
        vv = v.clone().requires_grad_(True)
        out = FlashAttentionFunction.apply(q, kk, vv, True, qoff)
        s = torch.matmul(q.float(), kk.float().transpose(-2, -1)) * scale
        mask = torch.ones(Tq, Tk, dtype=torch.bool, device="cuda").tril(qoff)
        ref = torch.matmul(torch.softmax(s.masked_fill(~mask, float("-inf")), -1), vv.float())
        assert (out.float() - ref).abs().max() < 2e-2, (r, (out.float() - ref).abs().max())
        g = torch.randn_like(out)
        out.backward(g)
        # reference grads via autograd on the fp32 path
        q2 = q.detach().float().requires_grad_(True)
        k2 = kk.detach().float().requires_grad_(True)
        v2 = vv.detach().float().requires_grad_(True)
        s2 = torch.matmul(q2, k2.transpose(-2, -1)) * scale
        r2 = torch.matmul(torch.softmax(s2.masked_fill(~mask, float("-inf")), -1), v2)
        r2.backward(g.float())
        assert (q.grad.float() - q2.grad).abs().max() < 5e-2
        assert (kk.grad.float() - k2.grad).abs().max() < 5e-2
        assert (vv.grad.float() - v2.grad).abs().max() < 5e-2


@pytest.mark.gpu
def test_fp8_linear_forward():
    """Experimental e4m3 forward: correct within fp8 rounding, bf16 grads."""
    from quintnet_amd.ops.linear import linear

    torch.manual_seed(5)
    x = torch.randn(256, 768, device="cuda", dtype=torch.bfloat16, requires_grad=True)
    w = torch.randn(512, 768, device="cuda", dtype=torch.bfloat16, requires_grad=True)
    b = torch.randn(512, device="cuda", dtype=torch.bfloat16)
    out = linear(x, w, b, fp8=True)
    ref = torch.nn.functional.linear(x.float(), w.float(), b.float())
    rel = (out.float() - ref).abs().mean() / ref.abs().mean()
    assert rel < 0.08, float(rel)
    out.sum().backward()
    assert x.grad is not None and w.grad is not None
    assert torch.isfinite(x.grad).all() and torch.isfinite(w.grad).all()


def test_ring_flash_chunks_match_direct():
    """Fused-flash per-chunk ring path (context_parallel): a single-rank
    simulation of the cp=2 chunk walk (diag chunk + one full chunk with
    streaming base-2 LSE merge, then per-chunk fused backward with the
    global lse2) must match the direct flash kernel with q_offset."""
    import math

    import torch

    from quintnet_amd.ops.attention import attention
    from quintnet_amd.parallel.context_parallel import (
        _ring_flash_bwd_hop,
        _ring_flash_fwd_hop,
    )

    torch.manual_seed(0)
    B, H, T, D = 2, 3, 512, 64
    Tl = T // 2
    dev = torch.device("cuda")
    q = torch.randn(B, H, T, D, device=dev, dtype=torch.bfloat16)
    k = torch.randn_like(q)
    v = torch.randn_like(q)
    scale = 1.0 / math.sqrt(D)

    # "rank 1" of cp=2: q shard = rows [Tl, 2Tl)
    qs = q[:, :, Tl:].contiguous()
    k0, v0 = k[:, :, :Tl].contiguous(), v[:, :, :Tl].contiguous()
    k1, v1 = k[:, :, Tl:].contiguous(), v[:, :, Tl:].contiguous()

    out_run = torch.zeros(B, H, Tl, D, device=dev)
    lse_run = torch.full((B, H, Tl, 1), float("-inf"), device=dev)
    # ring hop order: own (diagonal) chunk first, then the previous rank's
    out_run, lse_run = _ring_flash_fwd_hop(qs, k1, v1, scale, 1, out_run, lse_run)
    out_run, lse_run = _ring_flash_fwd_hop(qs, k0, v0, scale, 0, out_run, lse_run)
    out = out_run.to(qs.dtype)

    # reference: direct fused path over the full KV with q_offset
    qr = qs.clone().requires_grad_(True)
    kr = k.clone().requires_grad_(True)
    vr = v.clone().requires_grad_(True)
    ref = attention(qr, kr, vr, causal=True, q_offset=Tl)
    assert torch.allclose(out.float(), ref.float(), atol=2e-2, rtol=2e-2), (
        (out.float() - ref.float()).abs().max().item()
    )

    # backward: per-chunk fused kernels with the merged (global) lse2
    dout = torch.randn_like(out)
    ref.backward(dout)
    lse_flat = lse_run.reshape(B * H, Tl).contiguous()
    dq_acc = torch.zeros(B, H, Tl, D, device=dev)
    dk_all = torch.zeros(B, H, T, D, device=dev)
    dv_all = torch.zeros(B, H, T, D, device=dev)
    dqp = torch.empty_like(qs)
    dkp = torch.empty_like(qs)
    dvp = torch.empty_like(qs)
    for (kc, vc, diag, sl) in [(k1, v1, 1, slice(Tl, T)), (k0, v0, 0, slice(0, Tl))]:
        _ring_flash_bwd_hop(qs, kc, vc, out, dout, lse_flat, scale, diag,
                            dqp, dkp, dvp)
        dq_acc += dqp.float()
        dk_all[:, :, sl] += dkp.float()
        dv_all[:, :, sl] += dvp.float()

    assert torch.allclose(dq_acc, qr.grad.float(), atol=5e-2, rtol=5e-2), (
        (dq_acc - qr.grad.float()).abs().max().item()
    )
    assert torch.allclose(dk_all, kr.grad.float(), atol=5e-2, rtol=5e-2), (
        (dk_all - kr.grad.float()).abs().max().item()
    )
    assert torch.allclose(dv_all, vr.grad.float(), atol=5e-2, rtol=5e-2), (
        (dv_all - vr.grad.float()).abs().max().item()
    )


def test_zigzag_flash_world1_matches_direct():
    """world=1 zigzag (chunks (0,1), blocks diag/full/diag) through the
    FLASH branch must reproduce plain causal flash attention + grads."""
    import torch

    from quintnet_amd.ops.attention import attention
    from quintnet_amd.parallel.context_parallel import _ZigzagRingAttention

    torch.manual_seed(1)
    B, H, T, D = 2, 4, 512, 64  # h = 256 -> flash path engages
    dev = torch.device("cuda")
    q = torch.randn(B, H, T, D, device=dev, dtype=torch.bfloat16,
                    requires_grad=True)
    k = torch.randn_like(q).requires_grad_(True)
    v = torch.randn_like(q).requires_grad_(True)
    out = _ZigzagRingAttention.apply(q, k, v, None, True)
    qr = q.detach().clone().requires_grad_(True)
    kr = k.detach().clone().requires_grad_(True)
    vr = v.detach().clone().requires_grad_(True)
    ref = attention(qr, kr, vr, causal=True)
    assert torch.allclose(out.float(), ref.float(), atol=2e-2, rtol=2e-2)
    dout = torch.randn_like(out)
    out.backward(dout)
    ref.backward(dout)
    for a, b in ((q, qr), (k, kr), (v, vr)):
        assert torch.allclose(a.grad.float(), b.grad.float(), atol=5e-2,
                              rtol=5e-2), (a.grad - b.grad).abs().max()


def test_gelu_epilogue_gemm_numerics():
    """hipBLASLt GELU_AUX_BIAS epilogue (csrc/blaslt.cpp): out equals
    gelu_tanh(x@w.T+b), aux equals the pre-activation, and the full
    autograd path (fused act_bwd on the aux) matches an fp32 oracle.
    EXPERIMENTAL (opt-in like the feature itself): run with
    QN_GELU_EPI=1."""
    import os

    from quintnet_amd.ops import ext, has_ext, linear

    if os.environ.get("QN_GELU_EPI") != "1":
        pytest.skip("experimental epilogue path (enable with QN_GELU_EPI=1)")
    if not has_ext() or not hasattr(ext(), "gemm_bias_gelu_aux"):
        pytest.skip("extension without gemm_bias_gelu_aux")
    torch.manual_seed(3)
    M, K, N = 512, 768, 3072
    x = torch.randn(M, K, device=DEV, dtype=torch.bfloat16)
    w = torch.randn(N, K, device=DEV, dtype=torch.bfloat16) * 0.02
    b = torch.randn(N, device=DEV, dtype=torch.bfloat16)
    out, aux = ext().gemm_bias_gelu_aux(x, w, b)
    pre_ref = torch.nn.functional.linear(x.float(), w.float(), b.float())
    out_ref = torch.nn.functional.gelu(pre_ref, approximate="tanh")
    scale = max(float(pre_ref.abs().max()), 1.0)
    assert (aux.float() - pre_ref).abs().max() / scale < 3e-2
    assert (out.float() - out_ref).abs().max() / scale < 3e-2

    # end-to-end through LinearFunction (epilogue branch) vs fp32
    xg = x.clone().requires_grad_(True)
    wg = w.clone().requires_grad_(True)
    bg = b.clone().requires_grad_(True)
    y = linear(xg, wg, bg, activation="gelu")
    g = torch.randn_like(y)
    y.backward(g)
    xr = x.float().requires_grad_(True)
    wr = w.float().requires_grad_(True)
    br = b.float().requires_grad_(True)
    yr = torch.nn.functional.gelu(
        torch.nn.functional.linear(xr, wr, br), approximate="tanh"
    )
    yr.backward(g.float())
    for got, ref in ((xg.grad, xr.grad), (wg.grad, wr.grad), (bg.grad, br.grad)):
        s = max(float(ref.abs().max()), 1.0)
        assert (got.float() - ref).abs().max() / s < 5e-2
