"""GPU numerics of the one-pass LayerNorm backward (dx and the dw/db chunk
partials from a single read of dy and x) against an fp32 autograd reference,
on the shapes that take it and on the shapes that keep the two-kernel path."""

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    DEV = torch.device("cuda", 0)
else:
    pytest.skip("needs MI355X", allow_module_level=True)

BF16 = torch.bfloat16
ROUND = 16  # rows a block of the one-pass kernel stages per round


def _ext():
    from quintnet_amd.ops import ext, has_ext

    assert has_ext(), "HIP extension must be present on a GPU box"
    return ext()


def _tail_rows():
    """rows = 2*ROUND*chunks + 3: every block runs two full rounds, then a
    ragged one in which most waves own no row."""
    rows = 2 * ROUND + 3
    assert rows == 2 * ROUND * _ext().layernorm_bwd_chunks(rows) + 3
    return rows


def _ln_case(rows, h, dt, with_dsum, seed=0):
    torch.manual_seed(seed)
    x = torch.randn(rows, h, device=DEV, dtype=dt)
    w = torch.randn(h, device=DEV, dtype=dt)
    b = torch.randn(h, device=DEV, dtype=dt)
    dy = torch.randn(rows, h, device=DEV, dtype=dt)
    dsum = torch.randn(rows, h, device=DEV, dtype=dt) if with_dsum else None
    _, mean, rstd = _ext().layernorm_fwd(x, w, b, 1e-5, None)
    return x, w, b, dy, dsum, mean, rstd


def _check_ln(rows, h, dt, with_dsum):
    x, w, b, dy, dsum, mean, rstd = _ln_case(rows, h, dt, with_dsum)
    dx, dw, db = _ext().layernorm_bwd(dy, x, w, mean, rstd, dsum)
    xf = x.float().requires_grad_(True)
    wf = w.float().requires_grad_(True)
    bf = b.float().requires_grad_(True)
    rr = torch.nn.functional.layer_norm(xf, (h,), wf, bf, 1e-5)
    gx, gw, gb = torch.autograd.grad(rr, (xf, wf, bf), dy.float())
    if with_dsum:
        gx = gx + dsum.float()
    s = max(float(gx.abs().max()), 1.0)
    dx_tol = 3e-2 * s if dt == BF16 else 1e-4 * s
    assert dx.dtype == dt and dw.dtype == dt and db.dtype == dt
    assert dx.shape == x.shape and dw.shape == (h,) and db.shape == (h,)
    assert (dx.float() - gx).abs().max() < dx_tol
    assert (dw.float() - gw).abs().max() / max(float(gw.abs().max()), 1.0) < 3e-2
    assert (db.float() - gb).abs().max() / max(float(gb.abs().max()), 1.0) < 3e-2


@pytest.mark.parametrize("with_dsum", [False, True])
@pytest.mark.parametrize("h", [512, 768, 1024])
@pytest.mark.parametrize("rows", [1, 5, 1030, "tail"])
def test_layernorm_bwd_one_pass(rows, h, with_dsum):
    if rows == "tail":
        rows = _tail_rows()
    _check_ln(rows, h, BF16, with_dsum)


@pytest.mark.parametrize("with_dsum", [False, True])
@pytest.mark.parametrize("rows,h,dt", [(65, 100, torch.float32), (77, 3072, BF16)])
def test_layernorm_bwd_two_kernel_shapes(rows, h, dt, with_dsum):
    _check_ln(rows, h, dt, with_dsum)


def test_db_is_the_column_sum_of_dy():
    """db sums bf16 values in fp32: against the float sum of dy it may differ
    by one bf16 rounding of the result plus the fp32 reordering bound."""
    rows, h = 1030, 768
    x, w, b, dy, dsum, mean, rstd = _ln_case(rows, h, BF16, False, seed=2)
    _, _, db = _ext().layernorm_bwd(dy, x, w, mean, rstd, None)
    t = dy.float()
    ref = t.sum(0)
    bound = 2.0 ** -8 * ref.abs() + rows * 2.0 ** -24 * t.abs().sum(0)
    assert bool(((db.float() - ref).abs() <= bound).all())


@pytest.mark.parametrize("rows,h", [(4096, 768), (4096, 1024)])
def test_bit_reproducible(rows, h):
    x, w, b, dy, dsum, mean, rstd = _ln_case(rows, h, BF16, True, seed=3)
    r1 = _ext().layernorm_bwd(dy, x, w, mean, rstd, dsum)
    r2 = _ext().layernorm_bwd(dy, x, w, mean, rstd, dsum)
    for a, c in zip(r1, r2):
        assert torch.equal(a, c)


def test_dx_rows_do_not_depend_on_the_batch():
    """dx of a row is a function of that row alone: the same rows inside a
    larger call (other chunk and round assignment) give the same bits."""
    x, w, b, dy, dsum, mean, rstd = _ln_case(1030, 768, BF16, True, seed=4)
    dx_all, _, _ = _ext().layernorm_bwd(dy, x, w, mean, rstd, dsum)
    n = 37
    dx_head, _, _ = _ext().layernorm_bwd(
        dy[:n].contiguous(), x[:n].contiguous(), w, mean[:n].contiguous(),
        rstd[:n].contiguous(), dsum[:n].contiguous())
    assert torch.equal(dx_all[:n], dx_head)
