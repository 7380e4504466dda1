"""ops.decode_attention on CPU (the composed path): append + row-by-row
causal attention over a static cache, and the StaticKVDecoder switch."""

import pytest
import torch


def _reference(q, kc, vc, past, scale):
    """Row r attends cache rows [0, past + r], computed from scratch."""
    B, H, T, D = q.shape
    out = torch.empty_like(q)
    for r in range(T):
        n = past + r + 1
        s = torch.einsum("bhd,bhjd->bhj", q[:, :, r].float(), kc[:, :, :n].float())
        p = torch.softmax(s * scale, dim=-1)
        out[:, :, r] = torch.einsum("bhj,bhjd->bhd", p, vc[:, :, :n].float())
    return out


@pytest.mark.parametrize("past_as_tensor", [True, False])
@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("past", [0, 1, 7])
def test_decode_attention_cpu(past, T, past_as_tensor):
    from quintnet_amd.ops import decode_attention

    torch.manual_seed(past * 10 + T)
    B, H, D, Tmax = 2, 3, 16, 12
    qkv = torch.randn(B, T, 3 * H * D)

    def heads(t):
        return t.view(B, T, H, D).permute(0, 2, 1, 3)

    q, k, v = (heads(qkv[:, :, i * H * D:(i + 1) * H * D]) for i in range(3))
    kc = torch.randn(B, H, Tmax, D)
    vc = torch.randn(B, H, Tmax, D)
    kc0, vc0 = kc.clone(), vc.clone()
    p = torch.tensor(past) if past_as_tensor else past
    out = decode_attention(q, k, v, kc, vc, p)
    assert out.shape == (B, H, T, D)
    # the no-copy layout: [B, H, T, D] is a view of a [B, T, H*D] buffer
    assert out.permute(0, 2, 1, 3).is_contiguous()
    assert torch.equal(kc[:, :, past:past + T], k)
    assert torch.equal(vc[:, :, past:past + T], v)
    keep = torch.ones(Tmax, dtype=torch.bool)
    keep[past:past + T] = False
    assert torch.equal(kc[:, :, keep], kc0[:, :, keep])
    assert torch.equal(vc[:, :, keep], vc0[:, :, keep])
    want = _reference(q, kc, vc, past, 1.0 / D ** 0.5)
    torch.testing.assert_close(out, want, atol=1e-5, rtol=1e-5)
    # an explicit out view is filled in place
    kc2, vc2 = kc0.clone(), vc0.clone()
    buf = torch.empty(B, T, H * D)
    got = decode_attention(q, k, v, kc2, vc2, p, out=heads(buf))
    assert torch.equal(got, out) and torch.equal(heads(buf), out)


def test_decode_attention_rejects_overflow_on_host():
    from quintnet_amd.ops import decode_attention

    q = torch.randn(1, 1, 2, 8)
    kc = torch.zeros(1, 1, 4, 8)
    vc = torch.zeros(1, 1, 4, 8)
    with pytest.raises(AssertionError):
        decode_attention(q, q, q, kc, vc, 3)
    assert not kc.any() and not vc.any()


def test_static_decoder_fused_switch_cpu(monkeypatch):
    """fused_attention False / default / True decode the same tokens on CPU
    (config of test_static_decoder_matches_generate)."""
    from quintnet_amd.models import GPT2Config, GPT2Stage, StaticKVDecoder

    monkeypatch.delenv("QN_DECODE_ATTN", raising=False)
    torch.manual_seed(0)
    cfg = GPT2Config(n_embd=64, n_layer=3, n_head=2, vocab_size=128,
                     n_positions=96, dropout=0.0)
    stage = GPT2Stage(cfg).eval()
    ids = torch.randint(0, cfg.vocab_size, (2, 12))
    composed = StaticKVDecoder(stage, batch=2, max_len=96, fused_attention=False)
    default = StaticKVDecoder(stage, batch=2, max_len=96)
    forced = StaticKVDecoder(stage, batch=2, max_len=96, fused_attention=True)
    assert composed.fused_attention is False
    assert default.fused_attention is False  # no native kernel on CPU
    assert forced.fused_attention is True
    want = composed.generate(ids, max_new_tokens=10)
    assert torch.equal(default.generate(ids, max_new_tokens=10), want)
    assert torch.equal(forced.generate(ids, max_new_tokens=10), want)
    assert torch.equal(want, stage.generate(ids, max_new_tokens=10, temperature=0.0))
    monkeypatch.setenv("QN_DECODE_ATTN", "0")
    off = StaticKVDecoder(stage, batch=2, max_len=96, fused_attention=True)
    assert off.fused_attention is False
