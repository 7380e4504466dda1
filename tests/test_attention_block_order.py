"""The block-to-work mapping of the attention grids (csrc/attn.h:
attn_block_of), run on the host through the extension — no GPU needed.

For every nblk in 1..9 and BH in 1..20, in both orientations (q-major:
fwd and dq, heavy = high row block; key-major: dkv, heavy = low):
  a. L -> (blk, bh) is a bijection onto [0, nblk) x [0, BH);
  b. the block weight (causal tile count) is non-increasing in L;
  c. when BH % 8 == 0, the eight classes L % 8 (the XCDs: workgroups are
     dealt round-robin by linear id) hold equal total tile counts, and
     bh % 8 == L % 8 (a head's blocks share one XCD).
"""

import pytest

NBLK = range(1, 10)
BHS = range(1, 21)


@pytest.fixture(scope="module")
def C():
    from quintnet_amd import _C

    return _C


def _weight(blk, nblk, key_major):
    """32-wide tiles a causal block walks at Tq == Tk, q_offset == 0."""
    return 4 * (nblk - blk) if key_major else 4 * (blk + 1)


@pytest.mark.parametrize("key_major", [False, True], ids=["qmajor", "kvmajor"])
def test_balanced_order(C, key_major):
    order = C.attn_order_for(True, True, key_major)
    assert order != C.attn_order_for(False, True, key_major)
    for nblk in NBLK:
        for BH in BHS:
            tag = (nblk, BH, key_major)
            cells = [C.attn_block_of(L, nblk, BH, order) for L in range(nblk * BH)]
            # a. bijection
            assert all(0 <= blk < nblk and 0 <= bh < BH for blk, bh in cells), tag
            assert len(set(cells)) == nblk * BH, tag
            # the form the issue states
            for L, (blk, bh) in enumerate(cells):
                assert bh == L % BH, tag
                assert blk == (L // BH if key_major else nblk - 1 - L // BH), tag
            # b. heaviest first
            w = [_weight(blk, nblk, key_major) for blk, _ in cells]
            assert all(x >= y for x, y in zip(w, w[1:])), tag
            # c. equal load per XCD class, one XCD per head
            if BH % 8 == 0:
                per = [sum(w[L] for L in range(c, nblk * BH, 8)) for c in range(8)]
                assert len(set(per)) == 1, (tag, per)
                assert all(bh % 8 == L % 8 for L, (_, bh) in enumerate(cells)), tag


def test_linear_order_is_the_2d_grid(C):
    """linear, and every non-causal launch: block id x + nblk * y of a
    dim3(nblk, BH) grid."""
    for key_major in (False, True):
        order = C.attn_order_for(False, True, key_major)
        assert C.attn_order_for(True, False, key_major) == order
        assert C.attn_order_for(False, False, key_major) == order
        for nblk in NBLK:
            for BH in BHS:
                cells = [C.attn_block_of(L, nblk, BH, order) for L in range(nblk * BH)]
                assert cells == [(L % nblk, L // nblk) for L in range(nblk * BH)]


def test_linear_order_skew_at_the_xcd_count(C):
    """What the balanced order removes: at nblk == 8 the linear order gives
    each XCD class one row block only, a max/mean load of 32/18."""
    nblk, BH = 8, 16
    order = C.attn_order_for(False, True, False)
    w = [_weight(C.attn_block_of(L, nblk, BH, order)[0], nblk, False)
         for L in range(nblk * BH)]
    per = [sum(w[c::8]) for c in range(8)]
    assert max(per) * 18 == 32 * (sum(per) // 8)
