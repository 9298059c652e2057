"""GPU tests of the occupancy refresh (csrc/occupancy.hip): the device draw stream, the sample list, the EMA apply, the
re-binarisation and `OccGridEstimator._update` / `mnf_update_occupancy`, each held BIT FOR BIT to tests/occ_ref.py, the numpy
restatement of what include/mi355nerf.h documents (itself held to the Philox known answers, oracle/occgrid.py and the reference's
recorded trajectory by test_occ_ref_cpu.py).

The entry points are called through `_lib` exactly as nerfacc.py calls them.  Every output buffer is over-allocated and carries a
poisoned guard band behind it, which must come back untouched.  The only tolerance in this file is the 1 float32 ulp on the
threshold of a grid whose double sum depends on the summation order (test_binarize_arbitrary, test_fused_update_with_a_real_field);
everywhere else `assert_array_equal` on the bits."""
import ctypes
import functools
import itertools

import numpy as np
import pytest
import torch

import helpers as H
import occ_ref as OR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
AABB = np.array([-19.1, -0.2, -19.1, 0.5, 3.2, 0.5], np.float32)

# the smallest grids that reach each path
SMALL = [(2, 1, 2),        # 4 cells: N = 1, one partial word
         (1, 1, 3),        # 3 cells: N = 0, capacity 0 after the warm-up
         (5, 7, 3)]        # 105 cells: 4 words, 9 live bits in the last, non-cubic axis order
LARGE = [(13, 17, 11),     # 2431 cells: the second binarize group is partial, 76 words
         (40, 33, 27),     # 35 640 cells, 1114 words: the prefix carries into a second chunk
         (48, 48, 32)]     # 73 728 cells, 2304 words: two full chunks + 256, everything aligned
GRIDS = SMALL + LARGE
PATTERNS = ["none", "first", "last", "exactly_N", "N_plus_1", "all", "bernoulli_0.1", "bernoulli_0.6", "word_boundary"]
STEPS = [(0, 256), (255, 256), (256, 256), (4096, 256), (0, 0)]                 # (step, warmup_steps)
SEEDS = [0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 62 - 1, 2 ** 63 + 5]
_ids = lambda r: "x".join(str(v) for v in r)


def _lib():
    from apnrf_amd import _lib as L
    return L, L.load_library()


def _cu(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)            # (a copy: the shared states are read-only)


class Guarded:
    """n elements + GUARD poisoned ones behind them; `get()` returns the first n and asserts that the band is untouched"""
    POISON = {torch.int64: -7777, torch.float32: -77777.0, torch.uint8: 0xAB, torch.int32: 0x5A5A5A5A}

    def __init__(self, n, dtype, init=None):
        self.n, self.poison = int(n), self.POISON[dtype]
        self.t = torch.full((self.n + GUARD,), self.poison, dtype=dtype, device=DEV)
        if init is not None:
            self.t[:self.n] = _cu(init)

    @property
    def ptr(self):
        from apnrf_amd import _lib as L
        return L.ptr(self.t)

    def get(self):
        a = self.t.cpu().numpy()
        assert (a[self.n:] == np.asarray(self.poison, a.dtype)).all(), "guard band written"
        return a[:self.n]

    def untouched(self):
        a = self.t.cpu().numpy()
        return bool((a == np.asarray(self.poison, a.dtype)).all())


def _workspace(cells):
    L, lib = _lib()
    nbytes = int(lib.mnf_occ_workspace_bytes(cells, 0))
    assert nbytes > 0
    return Guarded(nbytes, torch.uint8), nbytes


def _c6(aabb):
    return (ctypes.c_float * 6)(*[float(v) for v in aabb])


def _pack_on_device(binaries_u8, cells, levels):
    """mnf_pack_bitgrid as `OccGridEstimator.bitgrid()` calls it -> (int32 device tensor [levels, words], its uint32 host copy)"""
    L, lib = _lib()
    words = (cells + 31) // 32
    bits = Guarded(levels * words, torch.int32)
    src = _cu(np.ascontiguousarray(binaries_u8, np.uint8).reshape(-1))
    L.launch(lib.mnf_pack_bitgrid, L.ptr(src), cells, levels, bits.ptr)
    return bits, bits.get().view(np.uint32).reshape(levels, words)


def _sample(occs_t, bits_t, res, aabb, step, warmup, seed, cap, ws, nbytes, idx_in=None, jit_in=None):
    """mnf_occ_sample_cells with guarded outputs -> (idx int64 [cap], points f32 [cap,3], the guarded idx buffer)"""
    L, lib = _lib()
    idx, pts = Guarded(cap, torch.int64), Guarded(3 * cap, torch.float32)
    n_in = 0 if idx_in is None else int(idx_in.shape[0])
    L.launch(lib.mnf_occ_sample_cells, L.ptr(occs_t), L.ptr(bits_t), res[0], res[1], res[2], _c6(aabb), int(step), int(warmup), int(seed),
             L.ptr(idx_in), L.ptr(jit_in), n_in, idx.ptr, pts.ptr, cap, ws.ptr, nbytes)
    return idx.get(), pts.get().reshape(cap, 3), idx


def _bits_equal(got, want, what=""):
    np.testing.assert_array_equal(np.ascontiguousarray(got, np.float32).view(np.uint32), np.ascontiguousarray(want, np.float32).view(np.uint32),
                                  err_msg=what)


# ------------------------------------------------------------------ states
def _boundary_word(cells):
    """the word whose neighbours straddle the most interesting boundary the grid has: the prefix kernel's 1024-word chunk, else a
    64-word wave, else word 1"""
    words = (cells + 31) // 32
    for w in (1024, 64, 1):
        if w + 1 < words:
            return w
    return 0


@functools.lru_cache(maxsize=None)
def _state(res, pattern):
    """(occs f32 [cells], binaries bool [cells]) — 10 % of the cells (at least one) carry occupancy -1, half of those taken from the
    occupied cells where there are any.  Nobody writes to the returned arrays."""
    cells = int(np.prod(res)); N = cells // 4
    rng = np.random.default_rng(cells * 16 + PATTERNS.index(pattern))
    b = np.zeros(cells, bool)
    if pattern == "first":
        b[0] = True
    elif pattern == "last":
        b[-1] = True
    elif pattern == "exactly_N":
        b[rng.permutation(cells)[:N]] = True
    elif pattern == "N_plus_1":
        b[rng.permutation(cells)[:N + 1]] = True
    elif pattern == "all":
        b[:] = True
    elif pattern.startswith("bernoulli"):
        b = rng.random(cells) < float(pattern.split("_")[1])
    elif pattern == "word_boundary":                  # one full word, bit 31 of the word before and bit 0 of the word after it
        w = _boundary_word(cells)
        lo, hi = max(32 * w - 1, 0), min(32 * w + 33, cells)
        b[lo:hi] = True
    occs = (rng.random(cells) * 0.02).astype(np.float32)
    n_neg = max(1, round(0.1 * cells))
    occupied, free = rng.permutation(np.nonzero(b)[0]), rng.permutation(np.nonzero(~b)[0])
    take = min(len(occupied), (n_neg + 1) // 2)
    neg = np.concatenate([occupied[:take], free[:n_neg - take]])
    if len(neg) < n_neg:
        neg = np.concatenate([neg, occupied[take:take + n_neg - len(neg)]])
    occs[neg] = -1.0
    occs.setflags(write=False); b.setflags(write=False)
    return occs, b


def _check_sample_case(res, pattern, step, warmup, seed, dev):
    cells = int(np.prod(res)); N = cells // 4
    occs, b = _state(res, pattern)
    occs_t, bits_t, ws, nbytes = dev
    cap = OR.list_capacity(cells, step, warmup)
    L, lib = _lib()
    assert int(lib.mnf_occ_list_capacity(cells, step, warmup)) == cap
    idx, pts, idx_buf = _sample(occs_t, bits_t, res, AABB, step, warmup, seed, cap, ws, nbytes)
    want_idx, want_pts = OR.sample_list(occs, b, res, AABB, step, warmup, seed)
    what = f"{res} {pattern} step {step}/{warmup} seed {seed}"
    np.testing.assert_array_equal(idx, want_idx, err_msg=what)
    _bits_equal(pts, want_pts, what)
    if cap == 0:
        assert idx_buf.untouched()
    # cells no camera sees: in the occupied half if occupied, never in the other halves
    neg = occs < 0
    if step >= warmup:
        uni, half = idx[:N], idx[N:]
        assert not neg[uni[uni >= 0]].any(), what
        if b.sum() <= N:
            assert set(np.nonzero(b & neg)[0]) <= set(half.tolist()), what
    else:
        assert not neg[idx[idx >= 0]].any(), what
    return idx, pts


def _device_state(res, pattern):
    cells = int(np.prod(res))
    occs, b = _state(res, pattern)
    bits, host = _pack_on_device(b.astype(np.uint8), cells, 1)
    np.testing.assert_array_equal(host, OR.pack_bits(b), err_msg=f"mnf_pack_bitgrid {res} {pattern}")
    ws, nbytes = _workspace(cells)
    return _cu(occs), bits.t, ws, nbytes


# ------------------------------------------------------------------ 1. the sample list from the device draws
@pytest.mark.parametrize("res", SMALL, ids=_ids)
def test_sample_list_small_grids_full_product(res):
    """every pattern x step x seed: cell_idx and points equal the restatement bit for bit"""
    for pattern in PATTERNS:
        dev = _device_state(res, pattern)
        got = {}
        for (step, warmup), seed in itertools.product(STEPS, SEEDS):
            got[(step, warmup, seed)] = _check_sample_case(res, pattern, step, warmup, seed, dev)
        dev[2].get()                                   # the band behind the workspace
        # two seeds that share their low word give different lists
        for step, warmup in STEPS:
            a, b = got[(step, warmup, 0)], got[(step, warmup, 2 ** 32)]
            if a[0].shape[0] and (a[0] >= 0).any():
                assert not np.array_equal(a[1], b[1]), f"{res} {pattern} step {step}: seed_hi has no effect"


def _large_cases():
    """about a dozen per grid: every pattern once past the warm-up (the three such step pairs and the seeds in rotation), and
    three warm-up lists"""
    past = [s for s in STEPS if s[0] >= s[1]]
    cases = [(p, past[i % len(past)], SEEDS[(i + 3) % len(SEEDS)]) for i, p in enumerate(PATTERNS)]
    cases += [("bernoulli_0.1", (0, 256), SEEDS[5]), ("all", (255, 256), SEEDS[2]), ("none", (0, 256), SEEDS[4])]
    return cases


@pytest.mark.parametrize("res", LARGE, ids=_ids)
def test_sample_list_large_grids(res):
    for pattern, (step, warmup), seed in _large_cases():
        dev = _device_state(res, pattern)
        a = _check_sample_case(res, pattern, step, warmup, seed, dev)
        other = seed ^ (1 << 32)                       # same low word
        b = _check_sample_case(res, pattern, step, warmup, other, dev)
        assert not np.array_equal(a[1], b[1]), f"{res} {pattern} step {step}: seed_hi has no effect"
        dev[2].get()


def test_sample_list_larger_capacity_leaves_the_rest_unused():
    """capacity above mnf_occ_list_capacity: the extra slots are -1 with the box centre, in both regimes"""
    res, cells = (5, 7, 3), 105
    dev = _device_state(res, "bernoulli_0.6")
    occs, b = _state(res, "bernoulli_0.6")
    for step in (0, 256):
        cap = OR.list_capacity(cells, step, 256) + 37
        idx, pts, _ = _sample(dev[0], dev[1], res, AABB, step, 256, 9, cap, dev[2], dev[3])
        want_idx, want_pts = OR.sample_list(occs, b, res, AABB, step, 256, 9, capacity=cap)
        np.testing.assert_array_equal(idx, want_idx); _bits_equal(pts, want_pts)
        assert (idx[-37:] == -1).all()


# ------------------------------------------------------------------ 2. explicit list
@pytest.mark.parametrize("res", GRIDS, ids=_ids)
def test_explicit_list(res):
    cells = int(np.prod(res))
    rng = np.random.default_rng(cells)
    dev = _device_state(res, "bernoulli_0.1")
    for n_in, cap in ((1, 2), (min(cells, 300), min(cells, 300) + 11), (2 * cells + 3, 2 * cells + 4)):
        ids = rng.integers(0, cells, n_in)
        if n_in > 2:
            ids[-1], ids[0] = cells - 1, 0
        jit = rng.random((n_in, 3)).astype(np.float32)
        idx, pts, _ = _sample(dev[0], dev[1], res, AABB, 300, 256, 5, cap, dev[2], dev[3], idx_in=_cu(ids), jit_in=_cu(jit))
        want_idx, want_pts = OR.explicit_list(ids, jit, res, AABB, cap)
        np.testing.assert_array_equal(idx, want_idx); _bits_equal(pts, want_pts, f"{res} n_in {n_in}")
        assert (idx[n_in:] == -1).all()
        centre = (AABB[:3] + AABB[3:]) * np.float32(0.5)
        _bits_equal(pts[n_in:], np.broadcast_to(centre, (cap - n_in, 3)))
    dev[2].get()


# ------------------------------------------------------------------ 3. apply
@pytest.mark.parametrize("scale, decay", [(1.0, 0.95), (1.0, 0.5), (1e-3, 0.95), (1e-3, 0.5)])
@pytest.mark.parametrize("res", GRIDS, ids=_ids)
def test_apply(res, scale, decay):
    """heavy duplication (4N entries over N/2 cells, unused slots in between), NaN candidates, NaN / negative / zero old values"""
    L, lib = _lib()
    cells = int(np.prod(res)); N = cells // 4
    rng = np.random.default_rng(cells + 7)
    pool = rng.permutation(cells)[:max(N // 2, 1)]
    n = max(4 * N, 8)
    ids = pool[rng.integers(0, len(pool), n)]
    ids[rng.random(n) < 0.05] = -1
    vals = (rng.standard_normal(n) * (0.02 / scale)).astype(np.float32)
    vals[rng.random(n) < 0.1] = np.nan
    occs = (rng.random(cells) * 0.03).astype(np.float32)
    kind = rng.random(cells)
    occs[kind < 0.1] = np.nan; occs[(kind >= 0.1) & (kind < 0.2)] = -1.0; occs[(kind >= 0.2) & (kind < 0.3)] = 0.0
    if len(pool) >= 3:
        occs[pool[0]], occs[pool[1]], occs[pool[2]] = np.nan, -1.0, 0.0
    jit = rng.random((n, 3)).astype(np.float32)
    ws, nbytes = _workspace(cells)
    occs_buf = Guarded(cells, torch.float32, init=occs)
    dummy_bits = torch.zeros((cells + 31) // 32, dtype=torch.int32, device=DEV)
    # the list goes through mnf_occ_sample_cells (explicit form) first, which builds the owner table in the shared workspace
    cap = n + 5
    idx, pts, idx_buf = _sample(occs_buf.t, dummy_bits, res, AABB, 300, 256, 0, cap, ws, nbytes, idx_in=_cu(ids), jit_in=_cu(jit))
    np.testing.assert_array_equal(idx[:n], ids)
    vals_full = np.concatenate([vals, np.full(5, 3.0, np.float32)])
    L.launch(lib.mnf_occ_apply, occs_buf.ptr, idx_buf.ptr, L.ptr(_cu(vals_full)), float(scale), cap, cells, float(decay), ws.ptr, nbytes)
    got = occs_buf.get()
    want = OR.apply(occs, idx, vals_full, scale, decay)
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32), err_msg=f"{res} scale {scale} decay {decay}")
    changed = got.view(np.uint32) != occs.view(np.uint32)
    assert (changed.any() or cells < 16) and not changed[np.setdiff1d(np.arange(cells), pool)].any()
    ws.get()


# ------------------------------------------------------------------ 4. binarize
def _binarize(occs, cells, levels, occ_thre):
    """mnf_occ_binarize with guarded outputs -> (binaries u8 [L,cells], bits u32 [L,words], thre f32); also checks that
    mnf_pack_bitgrid of the returned bytes gives the returned bits"""
    L, lib = _lib()
    words = (cells + 31) // 32
    ws, nbytes = _workspace(cells)
    binaries, bits, thre = Guarded(levels * cells, torch.uint8), Guarded(levels * words, torch.int32), Guarded(1, torch.float32)
    L.launch(lib.mnf_occ_binarize, L.ptr(_cu(occs)), cells, levels, float(occ_thre), binaries.ptr, bits.ptr, thre.ptr, ws.ptr, nbytes)
    b, w, t = binaries.get().reshape(levels, cells), bits.get().view(np.uint32).reshape(levels, words), thre.get()[0]
    ws.get()
    repacked = Guarded(levels * words, torch.int32)
    L.launch(lib.mnf_pack_bitgrid, binaries.ptr, cells, levels, repacked.ptr)
    np.testing.assert_array_equal(repacked.get().view(np.uint32).reshape(levels, words), w, err_msg="mnf_pack_bitgrid(binaries) != bitgrid")
    return b, w, t


def _dyadic_with_exact_mean(cells, levels, rng):
    """k * 2^-16, k <= 4096, 10 % at -1; the mean of the rest is exactly the value of one of them (cell `at`)"""
    total = cells * levels
    k = rng.integers(0, 4097, total)
    valid = np.ones(total, bool)
    valid[rng.permutation(total)[:max(1, round(0.1 * total))]] = False
    ids = np.nonzero(valid)[0]
    at, others = ids[len(ids) // 2], np.delete(ids, len(ids) // 2)
    m = len(others)
    if m:
        r = int(k[others].sum() % m)
        down, up = others[k[others] >= 1], others[k[others] < 4096]
        if len(down) >= r:
            k[down[:r]] -= 1
        else:
            assert len(up) >= m - r
            k[up[:m - r]] += 1
        assert k[others].sum() % m == 0
        k[at] = k[others].sum() // m
    occs = (k * 2.0 ** -16).astype(np.float32)
    occs[~valid] = -1.0
    return occs, int(at), np.float32(k[at] * 2.0 ** -16)


@pytest.mark.parametrize("levels", [1, 2, 3])
@pytest.mark.parametrize("res", GRIDS, ids=_ids)
def test_binarize_dyadic(res, levels):
    """occs on a dyadic grid: every summation order is exact in double, so threshold, bytes and bits are all bit-equal"""
    cells = int(np.prod(res))
    rng = np.random.default_rng(cells * 4 + levels)
    occs, at, mean = _dyadic_with_exact_mean(cells, levels, rng)
    # occ_thre above the mean: the threshold is the mean, and the cell equal to it is not occupied
    b, w, t = _binarize(occs, cells, levels, 1.0)
    want_b, want_w, want_t = OR.binarize(occs, cells, levels, 1.0)
    assert want_t == mean and t.view(np.uint32) == want_t.view(np.uint32), (t, want_t)
    np.testing.assert_array_equal(b, want_b); np.testing.assert_array_equal(w, want_w)
    assert b.reshape(-1)[at] == 0 and occs[at] == t
    # occ_thre below the mean: the threshold is occ_thre; one cell per level sits exactly on it
    on_cut = [lvl * cells + (cells - 1 if lvl % 2 else 0) for lvl in range(levels)]
    for cut in (np.float32(1024 * 2.0 ** -16), np.float32(2.0 ** -16)):          # (the second for a tiny grid whose mean is low)
        occs2 = occs.copy()
        occs2[on_cut] = cut
        if OR.exact_mean(occs2) > cut:
            break
    b, w, t = _binarize(occs2, cells, levels, float(cut))
    want_b, want_w, want_t = OR.binarize(occs2, cells, levels, float(cut))
    assert want_t == cut and t.view(np.uint32) == want_t.view(np.uint32), (t, want_t)
    np.testing.assert_array_equal(b, want_b); np.testing.assert_array_equal(w, want_w)
    assert not b.reshape(-1)[on_cut].any() and (b.any() or cells * levels < 16)
    # nothing qualifies: NaN threshold, nothing occupied
    b, w, t = _binarize(np.full(cells * levels, -1.0, np.float32), cells, levels, 0.01)
    assert np.isnan(t) and not b.any() and not w.any()


def _ulps(a, b):
    return abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32)))


@pytest.mark.parametrize("levels", [1, 2, 3])
@pytest.mark.parametrize("res", GRIDS, ids=_ids)
def test_binarize_arbitrary(res, levels):
    """arbitrary float32 occs: the threshold within 1 float32 ulp of the exact mean (the double sum's order is the kernel's own),
    the bytes exactly occs > that threshold, the bits exactly the packed bytes"""
    cells = int(np.prod(res))
    rng = np.random.default_rng(cells * 4 + levels + 100)
    occs = np.exp(rng.standard_normal(cells * levels) * 2 - 5).astype(np.float32)
    occs[rng.random(cells * levels) < 0.1] = -1.0
    occs[0] = 0.0
    mean = OR.exact_mean(occs)
    for occ_thre in (1e3, float(mean) * 0.37):
        b, w, t = _binarize(occs, cells, levels, occ_thre)
        print(f"{res} L{levels} occ_thre {occ_thre:.6g}: threshold {t!r} exact {mean!r}")
        if occ_thre > 1:
            assert t > 0 and _ulps(t, mean) <= 1, (t, mean)
        else:
            assert t.view(np.uint32) == np.float32(occ_thre).view(np.uint32)
        want_b, want_w = OR.binarize_at(occs, cells, levels, t)
        np.testing.assert_array_equal(b, want_b); np.testing.assert_array_equal(w, want_w)
        assert 0 < b.sum() < b.size or cells * levels < 16
        tail = (32 - cells % 32) % 32
        if tail:
            assert (w[:, -1] >> np.uint32(32 - tail) == 0).all()


# ------------------------------------------------------------------ 5. OccGridEstimator._update end to end
A, B, C = 0.71875, 1.3125, 0.59375                    # dyadic, so a Python float and a float32 are the same number
HIGH = 983 * 2.0 ** -16                               # ~0.015: above occ_thre = 0.01 once, below it after one halving
# (step, fraction of space at the high value, the high value, occ_thre): chosen so that the occupied count of the state each refresh
# reads goes 0 -> above N (warm-up) -> at most N (mean threshold, a few cells at 1.0) -> above N again (see test_update_end_to_end)
SCHEDULE = [(0, 0.625, HIGH, 0.01), (16, 0.625, HIGH, 0.01), (256, 0.09375, 1.0, 1.0), (272, 0.875, HIGH, 0.01), (288, 0.3125, HIGH, 0.01)]


def _analytic_np(p, frac, high):
    """an occupancy on the 2^-16 grid made of exactly rounded float32 operations only, the same in numpy and in torch"""
    p = np.asarray(p, np.float32)
    t = ((p[:, 0] * np.float32(A)).astype(np.float32) + (p[:, 1] * np.float32(B)).astype(np.float32)).astype(np.float32)
    t = (t + (p[:, 2] * np.float32(C)).astype(np.float32)).astype(np.float32)
    g = (t - np.floor(t)).astype(np.float32)
    low = ((np.floor(g * np.float32(16)) + np.float32(1)) * np.float32(2.0 ** -16)).astype(np.float32)
    return np.where(g < np.float32(frac), np.float32(high), low).astype(np.float32)


def _analytic_torch(x, frac, high):
    t = (x[:, 0] * A + x[:, 1] * B) + x[:, 2] * C
    g = t - torch.floor(t)
    low = (torch.floor(g * 16.0) + 1.0) * (2.0 ** -16)
    return torch.where(g < frac, torch.full_like(g, high), low)


def _seed_of(k):
    """the seed `_update` draws after torch.manual_seed(k)"""
    torch.manual_seed(k)
    seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    torch.manual_seed(k)
    return seed


@pytest.mark.parametrize("levels", [1, 3])
@pytest.mark.parametrize("res", [(5, 7, 3), (40, 33, 27)], ids=_ids)
def test_update_end_to_end(res, levels):
    """five refreshes through `_update` (per-level seeds, per-level boxes, one threshold over all levels): occs, binaries and
    bitgrid() equal the restatement after every step; ema_decay 0.5 and values on the 2^-16 grid keep every mean exact"""
    from apnrf_amd.nerfacc import OccGridEstimator
    cells = int(np.prod(res)); N = cells // 4
    est = OccGridEstimator(torch.from_numpy(AABB), resolution=list(res), levels=levels).to(DEV).train()
    aabbs = est.aabbs.cpu().numpy()
    occs, binaries = np.zeros(levels * cells, np.float32), np.zeros((levels, cells), np.uint8)
    read_counts = []
    for k, (step, frac, high, occ_thre) in enumerate(SCHEDULE):
        read_counts.append(binaries.sum(1))
        seed = _seed_of(100 + k)
        est._update(step=step, occ_eval_fn=lambda x: _analytic_torch(x, frac, high), occ_thre=occ_thre, ema_decay=0.5)
        occs, binaries, bits, thre, _ = OR.update(occs, binaries, res, aabbs, step, 256, seed, lambda p: _analytic_np(p, frac, high),
                                                  occ_thre=occ_thre, ema_decay=0.5)
        what = f"{res} L{levels} step {step}"
        np.testing.assert_array_equal(est.occs.cpu().numpy().view(np.uint32), occs.view(np.uint32), err_msg=what)
        np.testing.assert_array_equal(est.binaries.cpu().numpy().reshape(levels, cells), binaries.astype(bool), err_msg=what)
        np.testing.assert_array_equal(est.bitgrid().cpu().numpy().view(np.uint32), bits, err_msg=what)
        assert est.binaries.dtype == torch.bool and tuple(est.binaries.shape) == (levels,) + tuple(res)
    # the occupied count that the refreshes past the warm-up read crosses N in both directions, on every level
    r = np.array(read_counts)                          # [5, levels]
    print(f"{res} L{levels}: occupied cells read by each refresh {r.tolist()}, N = {N}")
    assert (r[0] == 0).all() and (r[2] > N).all() and (r[3] <= N).all() and (r[3] > 0).all() and (r[4] > N).all()


def test_update_with_an_empty_list():
    """three cells: N = 0, so past the warm-up the list has capacity 0 — nothing is sampled or applied, the grid is re-thresholded"""
    from apnrf_amd.nerfacc import OccGridEstimator
    res, cells = (1, 1, 3), 3
    for levels in (1, 2):
        est = OccGridEstimator(torch.from_numpy(AABB), resolution=list(res), levels=levels).to(DEV).train()
        aabbs = est.aabbs.cpu().numpy()
        occs, binaries = np.zeros(levels * cells, np.float32), np.zeros((levels, cells), np.uint8)
        for k, step in enumerate((0, 256)):
            seed = _seed_of(7 + k)
            calls = []
            est._update(step=step, occ_eval_fn=lambda x: (calls.append(1), _analytic_torch(x, 0.5, HIGH))[1], occ_thre=1.0, ema_decay=0.5)
            occs, binaries, bits, thre, _ = OR.update(occs, binaries, res, aabbs, step, 256, seed, lambda p: _analytic_np(p, 0.5, HIGH),
                                                      occ_thre=1.0, ema_decay=0.5)
            np.testing.assert_array_equal(est.occs.cpu().numpy().view(np.uint32), occs.view(np.uint32))
            np.testing.assert_array_equal(est.binaries.cpu().numpy().reshape(levels, cells), binaries.astype(bool))
            np.testing.assert_array_equal(est.bitgrid().cpu().numpy().view(np.uint32), bits)
            assert len(calls) == (levels if step == 0 else 0)


# ------------------------------------------------------------------ 6. the fused call with a real field
def test_fused_update_with_a_real_field():
    """`mnf_update_occupancy` through `FieldDensityOcc` on the small scene at steps 0 and 256; the restatement is driven with the
    field's density at the restated points.  occs bit-equal; binaries == occs > t with t the exact threshold or one of its two
    float32 neighbours (the kernel's double sum has its own order); every cell is compared."""
    from apnrf_amd.nerfacc import FieldDensityOcc, OccGridEstimator
    scene = H.make_scene()
    hip = H.hip_field(scene)
    step_size, occ_thre = 1e-3, 1.0                   # the threshold is the mean: about half of the cells sit on either side
    res, cells = [int(r) for r in scene["res"]], int(np.prod(scene["res"]))
    est = OccGridEstimator(torch.from_numpy(scene["aabb"]), resolution=res, levels=1).to(DEV).train()
    aabbs = est.aabbs.cpu().numpy()
    occs, binaries = np.zeros(cells, np.float32), np.zeros((1, cells), np.uint8)
    density = lambda p: hip.query_density(_cu(p)).cpu().numpy().reshape(-1)
    for k, step in enumerate((0, 256)):
        seed = _seed_of(40 + k)
        est._update(step=step, occ_eval_fn=FieldDensityOcc(hip, step_size), occ_thre=occ_thre)
        before = occs
        occs, _, _, _, lists = OR.update(occs, binaries, res, aabbs, step, 256, seed, density, occ_thre=occ_thre, ema_decay=0.95,
                                         value_scale=step_size)
        got = est.occs.cpu().numpy()
        np.testing.assert_array_equal(got.view(np.uint32), occs.view(np.uint32), err_msg=f"step {step}")
        assert (got != before).sum() > cells // 8 and not np.isnan(got).any()
        mean = OR.exact_mean(occs)
        got_b = est.binaries.cpu().numpy().reshape(1, cells)
        fits = []
        for cand in (mean, np.nextafter(mean, np.float32(-np.inf)), np.nextafter(mean, np.float32(np.inf))):
            t = min(np.float32(cand), np.float32(occ_thre))
            want_b, want_bits = OR.binarize_at(occs, cells, 1, t)
            fits.append(np.array_equal(got_b, want_b.astype(bool))
                        and np.array_equal(est.bitgrid().cpu().numpy().view(np.uint32), want_bits))
        print(f"step {step}: exact mean {mean!r}, occupied {int(got_b.sum())} of {cells}, fits (exact, below, above) {fits}")
        assert any(fits), f"step {step}"
        assert 0 < got_b.sum() < cells
        binaries = got_b.astype(np.uint8)              # the next refresh reads the device's grid
