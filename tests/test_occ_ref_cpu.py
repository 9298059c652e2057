"""tests/occ_ref.py, the numpy restatement of the occupancy refresh that tests/test_gpu_occupancy.py holds csrc/occupancy.hip to bit
for bit, is itself held here to what the repository already trusts: the published Philox4x32-10 known answers (Random123's
kat_vectors), a separately written scalar form, oracle/occgrid.py, and the reference's recorded trajectory
tests/golden/occgrid.npz.  No GPU."""
import numpy as np
import pytest

import occ_ref as OR
from oracle import occgrid as OG

KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def _philox_scalar(ctr, key):
    """Philox4x32-10 on Python integers, written from the paper's round description: (hi, lo) of two 32x32 products,
    out = (hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0), the key bumped by the Weyl constants after every round."""
    c0, c1, c2, c3 = (int(v) for v in ctr)
    k0, k1 = (int(v) for v in key)
    for _ in range(10):
        prod0, prod1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        hi0, lo0 = divmod(prod0, 1 << 32)
        hi1, lo1 = divmod(prod1, 1 << 32)
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + 0x9E3779B9) % (1 << 32), (k1 + 0xBB67AE85) % (1 << 32)
    return c0, c1, c2, c3


@pytest.mark.parametrize("ctr, key, want", KAT)
def test_philox_known_answers(ctr, key, want):
    assert _philox_scalar(ctr, key) == want
    got = OR.philox4x32_10(np.array([ctr], np.uint32), np.array(key, np.uint32))
    assert got.dtype == np.uint32 and got.shape == (1, 4)
    assert tuple(int(v) for v in got[0]) == want


def test_philox_vectorised_equals_scalar():
    rng = np.random.default_rng(0)
    ctr = rng.integers(0, 1 << 32, (1000, 4), dtype=np.uint64).astype(np.uint32)
    key = rng.integers(0, 1 << 32, (1000, 2), dtype=np.uint64).astype(np.uint32)
    got = OR.philox4x32_10(ctr, key)
    want = np.array([_philox_scalar(c, k) for c, k in zip(ctr.tolist(), key.tolist())], np.uint64).astype(np.uint32)
    np.testing.assert_array_equal(got, want)
    # one key for all counters
    got = OR.philox4x32_10(ctr[:50], key[3])
    want = np.array([_philox_scalar(c, key[3].tolist()) for c in ctr[:50].tolist()], np.uint64).astype(np.uint32)
    np.testing.assert_array_equal(got, want)


def test_draw_words_counter_and_key_layout():
    """counter (element, 0, kind, step), key (seed low, seed high)"""
    seed = (0x299f31d0 << 32) | 0xa4093822
    w = OR.draw_words(7, 1, 0x03707344, seed)
    for e in range(7):
        assert tuple(int(v) for v in w[e]) == _philox_scalar((e, 0, 1, 0x03707344), (0xa4093822, 0x299f31d0))


# ------------------------------------------------------------------ against oracle/occgrid.py
RES, AABB = (5, 7, 3), np.array([-19.1, -0.2, -19.1, 0.5, 3.2, 0.5], np.float32)


def _state(cells, seed, p_occ=0.3, p_neg=0.1):
    rng = np.random.default_rng(seed)
    occs = rng.random(cells).astype(np.float32) * np.float32(0.02)
    occs[rng.random(cells) < p_neg] = -1.0
    return occs, rng.random(cells) < p_occ


@pytest.mark.parametrize("res", [RES, (12, 5, 9), (1, 1, 3), (16, 16, 16)])
@pytest.mark.parametrize("step", [0, 256])
def test_sample_points_equal_the_oracle(res, step):
    cells = int(np.prod(res))
    occs, binaries = _state(cells, 3)
    idx, pts = OR.sample_list(occs, binaries, res, AABB, step, 256, seed=99)
    assert idx.shape == (OR.list_capacity(cells, step, 256),) and pts.shape == (idx.shape[0], 3) and pts.dtype == np.float32
    # the offsets the list was built from, once more
    N = cells // 4
    if step < 256:
        off = OR.unit_offsets(OR.draw_words(cells, 2, step, 99))
    else:
        off = np.concatenate([OR.unit_offsets(OR.draw_words(N, k, step, 99)) for k in (0, 1)]) if N else np.zeros((0, 3), np.float32)
    used = idx >= 0
    want = OG.cell_sample_points(idx[used], off[used], res, AABB)
    np.testing.assert_array_equal(pts[used].view(np.uint32), want.view(np.uint32))
    centre = (AABB[:3] + AABB[3:]) * np.float32(0.5)
    np.testing.assert_array_equal(pts[~used], np.broadcast_to(centre, (int((~used).sum()), 3)))
    # the same through the explicit form
    idx2, pts2 = OR.explicit_list(idx[used], off[used], res, AABB, capacity=int(used.sum()) + 3)
    np.testing.assert_array_equal(idx2[:-3], idx[used]); assert (idx2[-3:] == -1).all()
    np.testing.assert_array_equal(pts2[:-3].view(np.uint32), want.view(np.uint32))
    np.testing.assert_array_equal(pts2[-3:], np.broadcast_to(centre, (3, 3)))


@pytest.mark.parametrize("decay", [0.95, 0.5])
@pytest.mark.parametrize("dup", [False, True])
def test_apply_equals_the_oracle(decay, dup):
    rng = np.random.default_rng(5)
    cells = 300
    occs = (rng.random(cells).astype(np.float32) * np.float32(0.02)).astype(np.float32)
    occs[rng.random(cells) < 0.1] = -1.0
    occs[rng.random(cells) < 0.05] = np.nan
    idx = rng.integers(0, 40, 400) if dup else rng.permutation(cells)[:120]
    vals = (rng.standard_normal(idx.shape[0]) * 0.02).astype(np.float32)
    vals[rng.random(idx.shape[0]) < 0.15] = np.nan
    want = OG.ema_update(occs, idx, vals, decay)
    got = OR.apply(occs, idx, vals, 1.0, decay)
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    assert (got.view(np.uint32) != occs.view(np.uint32)).sum() > 10
    # unused slots in between change nothing
    holes = np.full(2 * idx.shape[0], -1, np.int64); holes[::2] = idx
    vals2 = np.full(holes.shape[0], 7.0, np.float32); vals2[::2] = vals
    np.testing.assert_array_equal(OR.apply(occs, holes, vals2, 1.0, decay).view(np.uint32), want.view(np.uint32))
    # value_scale multiplies the candidate in float32
    scaled = OR.apply(occs, idx, vals, 1e-3, decay)
    np.testing.assert_array_equal(scaled.view(np.uint32), OG.ema_update(occs, idx, vals * np.float32(1e-3), decay).view(np.uint32))


def _ulp_distance(a, b):
    return abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32)))


def test_binarize_equals_the_oracle_on_the_golden_states(golden):
    g = golden("occgrid")
    cells = int(np.prod(g["resolution"]))
    for k in range(5):
        occs = g[f"s{k}_occs"]
        want_bin, want_thre = OG.binarize(occs, 1e-2)
        binaries, bits, thre = OR.binarize(occs, cells, 1, 1e-2)
        assert binaries.shape == (1, cells) and binaries.dtype == np.uint8 and bits.shape == (1, (cells + 31) // 32) and bits.dtype == np.uint32
        assert _ulp_distance(thre, want_thre) <= 1, (k, thre, want_thre)      # the oracle's mean is a float32 pairwise sum
        clear = (occs != thre) & (occs != want_thre)
        np.testing.assert_array_equal(binaries[0][clear].astype(bool), want_bin[clear])
        np.testing.assert_array_equal(binaries[0][clear].astype(bool), g[f"s{k}_binaries"].reshape(-1)[clear])   # the reference's own
        assert clear.mean() > 0.99 and 0 < binaries.sum() < cells
        np.testing.assert_array_equal(OR.unpack_bits(bits[0], cells), binaries[0].astype(bool))


def _golden_draws(g, k, occs, binaries, cells):
    """cell list + offsets of golden step k from the reference's recorded RNG draws, as occ_grid.py:345-375 derives them"""
    step = int(g[f"s{k}_step"])
    draws = [g[[n for n in g.files if n.startswith(f"s{k}_draw{j}_")][0]] for j in range(int(g[f"s{k}_ndraws"]))]
    if step < 256:
        return step, np.arange(cells)[occs >= 0], draws[0]
    uni = draws[0]
    uni = uni[occs[uni] >= 0]
    occupied = np.nonzero(binaries)[0]
    if cells // 4 < len(occupied):
        return step, np.concatenate([uni, occupied[draws[1]]]), draws[2]
    return step, np.concatenate([uni, occupied]), draws[1]


def test_golden_trajectory_replayed_bit_for_bit(golden):
    """The reference's five recorded updates through explicit_list / apply / binarize, its occ_eval_fn evaluated by torch on the CPU as
    when the file was recorded: occs and binaries bit for bit."""
    import torch
    g = golden("occgrid")
    res = g["resolution"].tolist()
    cells = int(np.prod(res))

    def occ_eval_fn(p):
        x = torch.from_numpy(p)
        return ((torch.sin(x[:, :1] * 1.3) * torch.cos(x[:, 2:3] * 0.7) + 0.2 * x[:, 1:2]).clamp_min(0) * 0.02).numpy().reshape(-1)

    occs, binaries = np.zeros(cells, np.float32), np.zeros(cells, bool)
    for k in range(5):
        step, ids, jit = _golden_draws(g, k, occs, binaries, cells)
        idx, pts = OR.explicit_list(ids, jit, res, g["aabbs"][0], capacity=len(ids))
        occs = OR.apply(occs, idx, occ_eval_fn(pts), 1.0, 0.95)
        np.testing.assert_array_equal(occs.view(np.uint32), g[f"s{k}_occs"].view(np.uint32), err_msg=f"step {step}")
        b, bits, thre = OR.binarize(occs, cells, 1, 1e-2)
        binaries = b[0].astype(bool)
        clear = occs != thre
        np.testing.assert_array_equal(binaries[clear], g[f"s{k}_binaries"].reshape(-1)[clear], err_msg=f"step {step}")
        binaries = g[f"s{k}_binaries"].reshape(-1)


# ------------------------------------------------------------------ structure of the list
def test_binarize_threshold_strict_levels_and_tail_bits():
    cells, levels = 105, 3
    k = np.random.default_rng(2).integers(0, 4097, cells * levels)
    occs = (k * 2.0 ** -16).astype(np.float32)
    occs[::10] = -1.0
    sel = occs >= 0
    mean = np.float32(float(k[sel].sum()) * 2.0 ** -16 / sel.sum())
    b, bits, thre = OR.binarize(occs, cells, levels, 1.0)
    assert thre == mean
    np.testing.assert_array_equal(b.reshape(-1), occs > mean)
    # a cell equal to the threshold is not occupied; the cut applies to all levels alike
    cut = np.float32(1024 * 2.0 ** -16)
    occs[7], occs[cells + 33], occs[2 * cells + 104] = cut, cut, cut
    b, bits, thre = OR.binarize(occs, cells, levels, float(cut))
    assert thre == cut and b[0, 7] == 0 and b[1, 33] == 0 and b[2, 104] == 0 and 0 < b.sum() < b.size
    assert bits.shape == (3, 4) and (bits[:, 3] >> np.uint32(9) == 0).all()            # 105 = 96 + 9 live bits
    for lvl in range(levels):
        np.testing.assert_array_equal(OR.unpack_bits(bits[lvl], cells), b[lvl].astype(bool))
    b, bits, thre = OR.binarize(np.full(cells * levels, -1.0, np.float32), cells, levels, 0.01)
    assert np.isnan(thre) and not b.any() and not bits.any()


@pytest.mark.parametrize("res", [(2, 1, 2), (5, 7, 3), (13, 17, 11)])
def test_occupied_half(res):
    cells = int(np.prod(res)); N = cells // 4
    rng = np.random.default_rng(cells)
    occs = np.zeros(cells, np.float32); occs[::3] = -1.0
    for n_occ in sorted({0, 1, max(N - 1, 0), N, N + 1, cells}):
        binaries = np.zeros(cells, bool); binaries[rng.permutation(cells)[:n_occ]] = True
        idx, pts = OR.sample_list(occs, binaries, res, AABB, 300, 256, seed=5)
        idx_b, pts_b = OR.sample_list(occs, OR.pack_bits(binaries)[0], res, AABB, 300, 256, seed=5)
        np.testing.assert_array_equal(idx, idx_b); np.testing.assert_array_equal(pts, pts_b)
        half = idx[N:]
        if n_occ <= N:                                  # ascending and complete, cells with occs < 0 included
            np.testing.assert_array_equal(half[:n_occ], np.nonzero(binaries)[0])
            assert (half[n_occ:] == -1).all()
        else:                                           # N draws below n_occ into the ascending list
            assert (half >= 0).all() and binaries[half].all()
            pick = OR.scaled_pick(OR.draw_words(N, 1, 300, 5)[:, 0], n_occ)
            assert (pick < n_occ).all() and (pick >= 0).all()
            np.testing.assert_array_equal(half, np.nonzero(binaries)[0][pick])
        uni = idx[:N]
        assert (occs[uni[uni >= 0]] >= 0).all()          # the uniform half drops the cells no camera sees


def test_uniform_half_fills_its_bins_and_offsets_are_unit():
    res = (64, 64, 64)                                   # N = 2^16 draws
    cells = 64 ** 3
    idx, pts = OR.sample_list(np.zeros(cells, np.float32), np.zeros(cells, bool), res, AABB, 256, 256, seed=2 ** 40 + 17)
    uni = idx[:cells // 4]
    assert uni.shape[0] == 2 ** 16 and (uni >= 0).all() and (uni < cells).all() and (idx[cells // 4:] == -1).all()
    counts = np.bincount(uni // (cells // 64), minlength=64)
    sigma = np.sqrt(2 ** 16 * (1 / 64) * (63 / 64))
    assert np.abs(counts - 1024).max() < 5 * sigma, counts
    for kind in (0, 1, 2):
        u = OR.unit_offsets(OR.draw_words(2 ** 16, kind, 256, 12345))
        assert u.dtype == np.float32 and (u >= 0).all() and (u < 1).all()
        assert np.abs(u.mean(0) - 0.5).max() < 5 * np.sqrt(1 / 12 / 2 ** 16)
    lo, hi = AABB[:3], AABB[3:]
    assert (pts >= lo).all() and (pts <= hi).all()


def test_list_depends_on_step_kind_and_both_seed_words():
    base = dict(n=64, kind=0, step=300, seed=(7 << 32) | 9)
    ref = OR.draw_words(**base)
    for change in (dict(step=301), dict(kind=1), dict(kind=2), dict(seed=(7 << 32) | 10), dict(seed=(8 << 32) | 9)):
        other = OR.draw_words(**{**base, **change})
        assert (other != ref).mean() > 0.99, change      # every word of every element changes, bar chance
    res = (5, 7, 3)
    occs, binaries = _state(105, 1, p_occ=0.6)
    a = OR.sample_list(occs, binaries, res, AABB, 300, 256, (7 << 32) | 9)
    for step, seed in ((301, (7 << 32) | 9), (300, (7 << 32) | 10), (300, (8 << 32) | 9)):
        b = OR.sample_list(occs, binaries, res, AABB, step, 256, seed)
        assert not np.array_equal(a[0], b[0]) and not np.array_equal(a[1], b[1])
    # the two halves and the warm-up list are three different streams
    w = [OR.unit_offsets(OR.draw_words(26, k, 300, 1)) for k in (0, 1, 2)]
    assert not np.array_equal(w[0], w[1]) and not np.array_equal(w[0], w[2]) and not np.array_equal(w[1], w[2])
    # seeds wrap at 2^64 as a uint64 does
    np.testing.assert_array_equal(OR.draw_words(4, 0, 1, 2 ** 64 + 3), OR.draw_words(4, 0, 1, 3))


def test_update_chains_levels_with_seed_plus_level():
    res, levels = (5, 7, 3), 3
    cells = 105
    aabbs = np.stack([OG.enlarge_aabb(AABB, 2 ** l) for l in range(levels)])
    rng = np.random.default_rng(4)
    occs = (rng.integers(0, 4097, cells * levels) * 2.0 ** -16).astype(np.float32)
    binaries = rng.random((levels, cells)) < 0.4
    fn = lambda p: (np.floor(np.abs(p).sum(-1) * 64) * 2.0 ** -16).astype(np.float32)
    new, b, bits, thre, lists = OR.update(occs, binaries, res, aabbs, 300, 256, 1000, fn, occ_thre=1.0, ema_decay=0.5)
    want = occs.reshape(levels, cells).copy()
    for lvl in range(levels):
        idx, pts = OR.sample_list(want[lvl], binaries[lvl], res, aabbs[lvl], 300, 256, 1000 + lvl)
        np.testing.assert_array_equal(idx, lists[lvl][0]); np.testing.assert_array_equal(pts, lists[lvl][1])
        want[lvl] = OR.apply(want[lvl], idx, fn(pts), 1.0, 0.5)
    np.testing.assert_array_equal(new, want.reshape(-1))
    b2, bits2, thre2 = OR.binarize(new, cells, levels, 1.0)
    np.testing.assert_array_equal(b, b2); np.testing.assert_array_equal(bits, bits2); assert thre == thre2
    assert not np.array_equal(lists[0][0], lists[1][0])
