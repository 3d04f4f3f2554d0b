"""tests/nonfinite_ref.py against the float64 reference it restates, and the caps that keep the GPU properties of
tests/test_nonfinite_gpu.py from passing vacuously.  CPU only."""
import pytest
import torch

import nonfinite_ref as nf


def _weights(cout, cin, seed):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(cout, cin, 3, 3, generator=g, dtype=torch.float64)
    return torch.where(w.abs() < 1e-3, torch.full_like(w, 0.5), w)             # all nonzero: every tap carries the poison


def _poisoned(n, c, H, W, pos, ch, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(n, c, H, W, generator=g, dtype=torch.float64)
    p = torch.zeros(n, H, W, dtype=torch.bool)
    for i, r, col in pos:
        x[i, ch, r, col] = float("nan")
        p[i, r, col] = True
    return x, p


H, W = 7, 9
SPOTS = [(0, 0, 0), (0, 0, W - 1), (0, H - 1, 0), (0, H - 1, W - 1), (1, 0, 0), (0, 0, 4), (0, 3, 0), (0, H - 1, 5), (0, 2, W - 1), (0, 3, 4)]


@pytest.mark.parametrize("pos", SPOTS)
@pytest.mark.parametrize("relu", [False, True])
def test_reach_of_a_1x1_tile_is_the_references_nan_set(pos, relu):
    """Corners, edges, the interior and both sides of the seam between two images: with all weights nonzero the float64 convolution is
    NaN exactly on the clipped 3 x 3 dilation - in every output channel, in no other image - and torch.relu keeps it."""
    x, p = _poisoned(2, 3, H, W, [pos], ch=1)
    y = nf.conv_ref(x, _weights(4, 3, 1), torch.ones(4, dtype=torch.float64), relu)
    want = nf.reach(p, H, W, (1, 1))
    assert want.any() and not want[1 - pos[0]].any()
    for c in range(4):
        assert torch.equal(torch.isnan(y[:, c]), want)
    assert torch.isfinite(y[1 - pos[0]]).all()


def test_two_poisons_across_the_image_seam_do_not_meet():
    x, p = _poisoned(2, 1, H, W, [(0, H - 1, W - 1), (1, 0, 0)], ch=0)
    y = nf.conv_ref(x, _weights(2, 1, 2))
    want = nf.reach(p, H, W, (1, 1))
    assert torch.equal(torch.isnan(y[:, 0]), want)
    assert int(want[0].sum()) == 4 and int(want[1].sum()) == 4 and torch.equal(want[0].flip(0, 1), want[1])


def test_relu_keeps_nan_and_drops_minus_inf():
    """The reference's ReLU: NaN stays, -Inf becomes 0, +Inf stays - and the masked layer is a select, not a product."""
    v = torch.tensor([float("nan"), float("-inf"), float("inf"), -1.0, 2.0], dtype=torch.float64)
    r = torch.relu(v)
    assert torch.isnan(r[0]) and r[1] == 0 and r[2] == float("inf") and r[3] == 0 and r[4] == 2
    x, p = _poisoned(1, 1, H, W, [(0, 3, 4)], ch=0)
    mask = torch.zeros(1, 2, H, W, dtype=torch.bool)
    mask[:, 0] = True
    y = nf.conv_ref(x, _weights(2, 1, 3), mask=mask)
    assert torch.equal(torch.isnan(y[:, 0]), nf.reach(p, H, W, (1, 1))) and bool((y[:, 1] == 0).all())


@pytest.mark.parametrize("tile", [(1, 2), (2, 2), (4, 4)])
def test_larger_tiles_reach_a_superset_made_of_whole_tiles(tile):
    th, tw = tile
    for pos in SPOTS:
        p = torch.zeros(2, H, W, dtype=torch.bool)
        p[pos] = True
        small, big = nf.reach(p, H, W, (1, 1)), nf.reach(p, H, W, tile)
        assert bool((big | ~small).all()) and not big[1 - pos[0]].any()
        for r in range(0, H, th):                                # whole tiles or nothing
            for c in range(0, W, tw):
                t = big[pos[0], r:r + th, c:c + tw]
                assert bool(t.all()) or not bool(t.any())
                assert bool(t.all()) == bool(small[pos[0], r:r + th, c:c + tw].any())


def test_reach_of_a_run_of_layers_grows_by_one_dilation_per_layer():
    p = torch.zeros(1, 9, 11, dtype=torch.bool)
    p[0, 4, 5] = True
    r3 = nf.reach(p, 9, 11, (1, 1), layers=3)
    assert int(r3.sum()) == 49 and bool(r3[0, 1:8, 2:9].all())
    x = torch.rand(1, 2, 9, 11, dtype=torch.float64)
    x[0, 1, 4, 5] = float("nan")
    w = _weights(2, 2, 4)
    assert torch.equal(torch.isnan(nf.stack_ref(x, [(w, None, True)] * 3)[:, 0]), r3)


def test_ffdnet_edge_reaches_follow_the_resolution_change():
    """Head: the four full-resolution pixels of a half-resolution position poison that position's window; tail: a half-resolution
    position's window is a block of 2 x 2 pixels per position - both against the float64 layers themselves."""
    Hh, Wh = 5, 6
    g = torch.Generator().manual_seed(7)
    for r, c in [(0, 0), (3, 4), (2 * Hh - 1, 2 * Wh - 1), (4, 7)]:
        x = torch.rand(2, 1, 2 * Hh, 2 * Wh, generator=g, dtype=torch.float64)
        x[0, 0, r, c] = float("nan")
        p = torch.zeros(2, 2 * Hh, 2 * Wh, dtype=torch.bool)
        p[0, r, c] = True
        y = nf.ffdnet_head_ref(x, torch.tensor([0.1, 0.2]), _weights(3, 5, 5))
        assert torch.equal(torch.isnan(y[:, 2]), nf.reach_head(p, Hh, Wh, (1, 1)))
    h = torch.rand(2, 4, Hh, Wh, generator=g, dtype=torch.float64)
    h[1, 2, 0, Wh - 1] = float("nan")
    p = torch.zeros(2, Hh, Wh, dtype=torch.bool)
    p[1, 0, Wh - 1] = True
    y = nf.tail_ref(h, _weights(4, 4, 6), shuffle=True)
    want = nf.reach_tail(p, Hh, Wh, (1, 1))
    assert tuple(want.shape) == (2, 2 * Hh, 2 * Wh) and torch.equal(torch.isnan(y[:, 0]), want) and int(want.sum()) == 16
    # the folded bias + ReLU in front of the tail keeps the NaN where it is
    y = nf.tail_ref(h, _weights(4, 4, 6), in_bias=torch.ones(4, dtype=torch.float64), shuffle=True)
    assert torch.equal(torch.isnan(y[:, 0]), want)


def test_pack_mask_is_relu_mask_packs_word():
    bits = torch.zeros(1, 64, 1, 3, dtype=torch.bool)
    bits[0, 0, 0, 0] = bits[0, 63, 0, 1] = True
    bits[0, :, 0, 2] = True
    assert nf.pack_mask(bits).tolist() == [[[1, -(1 << 63), -1]]]


@pytest.mark.parametrize("name", sorted(nf.CASES))
def test_every_gpu_case_obeys_the_caps(name):
    """No property of the GPU file may pass vacuously: every run poisons exactly one pixel of one image (so another image has none), the
    reach is never empty, leaves at least half of the poisoned image alone and never touches another image; the positions hold the four
    corners, both sides of the image seam and both sides of every tiling seam inside the shape; the shape is ragged against the tile and
    the block tile in both directions and odd in width."""
    c = nf.CASES[name]
    n, Hc, Wc = c["shape"]
    th, tw = c["tile"]
    pos = nf.case_positions(name)
    assert n >= 2 and len(set(pos)) == len(pos)
    if name != "head_mfma":                                          # (the big launch: one poison set at a seam corner, on the existing shape)
        assert Wc % 2 == 1
        assert {(0, 0, 0), (0, 0, Wc - 1), (0, Hc - 1, 0), (0, Hc - 1, Wc - 1), (1, 0, 0)} <= set(pos)
        for s in c["rows"]:
            assert (0 < s < Hc) and any(p[1] == s - 1 for p in pos) and any(p[1] == s for p in pos)
        for s in c["cols"]:
            assert (0 < s < Wc) and any(p[2] == s - 1 for p in pos) and any(p[2] == s for p in pos)
        assert Hc % max(c["rows"]) and Wc % max(c["cols"]) and (th == 1 or Hc % th) and (tw == 1 or Wc % tw)
        assert Hc > max(c["rows"]) and Wc > max(c["cols"])           # more than one block in both directions
    for p in pos:
        poison = nf.case_poison(name, p)
        assert int(poison.sum()) == 1 and bool(poison[p[0]].any())
        r = nf.case_reach(name, poison)
        f = 2 if c["dst"] == "full" else 1
        assert tuple(r.shape) == (n, f * Hc, f * Wc)
        assert bool(r[p[0]].any()) and 2 * int(r[p[0]].sum()) <= r[p[0]].numel()
        others = [i for i in range(n) if i != p[0]]
        assert others and not bool(r[others].any())
