"""The yardstick of the occupancy-refresh tests: a numpy restatement of the refresh that include/mi355nerf.h documents
(`mnf_occ_sample_cells` -> occ_eval_fn -> `mnf_occ_apply` per level, then `mnf_occ_binarize` over all levels), i.e. of
`OccGridEstimator._update` (nerfacc/estimators/occ_grid.py:345-437) with the device's documented draw stream in place of the
torch RNG.  Pure numpy: no torch, no GPU, no package import.  Everything here is meant to be held to BIT equality.

The draw stream: Philox4x32-10 (Salmon et al., SC'11; Random123), counter (element, 0, kind, step), key (seed low, seed high);
kind 0 = uniform half, 1 = occupied half, 2 = warm-up.  Word 0 picks the cell, floor(w0 * n / 2^32) with n = cells (uniform) or the
number of occupied cells (occupied half, only when there are more than N = cells // 4 of them); words 1..3 are the in-cell offsets
(w & 0xFFFFFF) * 2^-24 along x, y, z.

Held to what the repository already trusts by test_occ_ref_cpu.py: the published Philox known answers, oracle/occgrid.py and the
reference's recorded trajectory tests/golden/occgrid.npz."""
import math

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57          # Philox4x32 multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85          # Weyl increments of the key
KIND_UNIFORM, KIND_OCCUPIED, KIND_WARMUP = 0, 1, 2
_LOW32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(ctr, key):
    """ctr [n,4] uint32, key [2] or [n,2] uint32 -> [n,4] uint32.  Ten rounds; the products are formed in uint64."""
    c = np.asarray(ctr, np.uint32).astype(np.uint64).reshape(-1, 4)
    k = np.broadcast_to(np.asarray(key, np.uint32).astype(np.uint64).reshape(-1, 2), (c.shape[0], 2))
    c0, c1, c2, c3 = c[:, 0], c[:, 1], c[:, 2], c[:, 3]
    k0, k1 = k[:, 0].copy(), k[:, 1].copy()
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & _LOW32, (p0 >> _S32) ^ c3 ^ k1, p0 & _LOW32
        k0, k1 = (k0 + np.uint64(W0)) & _LOW32, (k1 + np.uint64(W1)) & _LOW32
    return np.stack([c0, c1, c2, c3], -1).astype(np.uint32)


def draw_words(n, kind, step, seed):
    """The four words of elements 0 .. n-1 of one stream: counter (element, 0, kind, step), key (seed & 0xFFFFFFFF, seed >> 32)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    ctr = np.zeros((n, 4), np.uint32)
    ctr[:, 0] = np.arange(n, dtype=np.uint64).astype(np.uint32)
    ctr[:, 2] = kind
    ctr[:, 3] = np.uint32(int(step) & 0xFFFFFFFF)
    return philox4x32_10(ctr, np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint32))


def unit_offsets(words):
    """words [n,4] -> [n,3] f32 in [0, 1): (w & 0xFFFFFF) * 2^-24 of words 1..3 (exact in float32)."""
    return ((words[:, 1:4] & np.uint32(0xFFFFFF)).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)


def scaled_pick(w0, n):
    """floor(w0 * n / 2^32) -> int64"""
    return ((np.asarray(w0, np.uint32).astype(np.uint64) * np.uint64(n)) >> _S32).astype(np.int64)


def list_capacity(cells, step, warmup_steps):
    return cells if step < warmup_steps else 2 * (cells // 4)


def unpack_bits(bits, cells):
    """uint32 [words] -> bool [cells] (bit c & 31 of word c >> 5)"""
    b = np.asarray(bits).view(np.uint32).reshape(-1)
    return (((b[:, None] >> np.arange(32, dtype=np.uint32)) & np.uint32(1)).reshape(-1)[:cells]).astype(bool)


def pack_bits(binaries):
    """bool / u8 [L, cells] -> uint32 [L, ceil(cells / 32)], the tail bits of the last word zero"""
    b = np.asarray(binaries).astype(bool)
    b = b.reshape(1, -1) if b.ndim == 1 else b.reshape(b.shape[0], -1)
    levels, cells = b.shape
    words = (cells + 31) // 32
    padded = np.zeros((levels, words * 32), np.uint64)
    padded[:, :cells] = b
    return (padded.reshape(levels, words, 32) << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)


def points_of(idx, offsets, res, aabb):
    """occ_grid.py:395-401 with every operation rounded to float32 on its own; x is the slowest axis, z the fastest.
    Slots with idx < 0 carry the box centre (lo + hi) * 0.5."""
    idx = np.asarray(idx, np.int64)
    u = np.asarray(offsets, np.float32).reshape(-1, 3)
    res = [int(r) for r in res]
    aabb = np.asarray(aabb, np.float32)
    lo, hi = aabb[:3], aabb[3:]
    c = np.where(idx >= 0, idx, 0)
    coord = np.stack([c // (res[1] * res[2]), (c // res[2]) % res[1], c % res[2]], -1).astype(np.float32)
    x = ((coord + u).astype(np.float32) / np.asarray(res, np.float32)).astype(np.float32)
    pts = (lo + (x * (hi - lo).astype(np.float32)).astype(np.float32)).astype(np.float32)
    centre = ((lo + hi).astype(np.float32) * np.float32(0.5)).astype(np.float32)
    return np.where((idx >= 0)[:, None], pts, centre[None]).astype(np.float32)


def sample_list(occs, bits_or_binaries, res, aabb, step, warmup_steps, seed, capacity=None):
    """(idx int64 [cap], pts f32 [cap,3]) of one level.  occs [cells] f32; bits_or_binaries: the level's binaries (bool / u8 [cells] or
    [X,Y,Z]) or its packed words (uint32 / int32), unused during warm-up; cap = list_capacity(...) unless a larger `capacity` is given,
    whose extra slots are unused."""
    occs = np.asarray(occs, np.float32).reshape(-1)
    cells = int(np.prod([int(r) for r in res]))
    assert occs.shape[0] == cells
    need = list_capacity(cells, step, warmup_steps)
    cap = need if capacity is None else int(capacity)
    assert cap >= need
    idx = np.full(cap, -1, np.int64)
    off = np.zeros((cap, 3), np.float32)
    with np.errstate(invalid="ignore"):
        eligible = occs >= 0                                    # NaN is not eligible
    if step < warmup_steps:
        w = draw_words(cells, KIND_WARMUP, step, seed)
        idx[:cells] = np.where(eligible, np.arange(cells), -1)
        off[:cells] = unit_offsets(w)
    else:
        N = cells // 4
        b = np.asarray(bits_or_binaries)
        binaries = unpack_bits(b, cells) if b.dtype in (np.uint32, np.int32) else b.reshape(-1).astype(bool)
        assert binaries.shape[0] == cells
        if N > 0:
            w = draw_words(N, KIND_UNIFORM, step, seed)
            pick = scaled_pick(w[:, 0], cells)
            idx[:N] = np.where(eligible[pick], pick, -1)
            off[:N] = unit_offsets(w)
            w = draw_words(N, KIND_OCCUPIED, step, seed)
            occupied = np.nonzero(binaries)[0]
            n_occ = len(occupied)
            if n_occ <= N:
                idx[N:N + n_occ] = occupied                     # all of them, ascending (torch.nonzero of the flat grid); not filtered by occs
            else:
                idx[N:2 * N] = occupied[scaled_pick(w[:, 0], n_occ)]
            off[N:2 * N] = unit_offsets(w)
    return idx, points_of(idx, off, res, aabb)


def explicit_list(indices_in, jitter_in, res, aabb, capacity):
    """The list of a caller-provided draw (`indices_in`, `jitter_in` [n_in,3]): used as given, the remaining slots unused."""
    indices_in = np.asarray(indices_in, np.int64)
    n = indices_in.shape[0]
    assert n <= capacity
    idx = np.full(capacity, -1, np.int64)
    off = np.zeros((capacity, 3), np.float32)
    idx[:n] = indices_in
    off[:n] = np.asarray(jitter_in, np.float32).reshape(n, 3)
    return idx, points_of(idx, off, res, aabb)


def apply(occs, idx, values, value_scale=1.0, ema_decay=0.95):
    """occ_grid.py:403-434 for one level -> new occs [cells] f32.  A cell named several times is written by its highest list position
    only; the written value is max(old * decay, value * scale), every product rounded to float32; a NaN candidate or a NaN old value
    leaves the cell as it was (the roll-back from `occs_backup`)."""
    occs = np.asarray(occs, np.float32).copy()
    idx = np.asarray(idx, np.int64)
    values = np.asarray(values, np.float32).reshape(-1)
    assert values.shape[0] == idx.shape[0]
    owner = np.full(occs.shape[0], -1, np.int64)
    used = np.nonzero(idx >= 0)[0]
    np.maximum.at(owner, idx[used], used)
    cell = np.nonzero(owner >= 0)[0]
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        cand = (values[owner[cell]] * np.float32(value_scale)).astype(np.float32)
        old = occs[cell]
        new = np.maximum((old * np.float32(ema_decay)).astype(np.float32), cand)
    write = ~(np.isnan(cand) | np.isnan(old))
    occs[cell[write]] = new[write]
    return occs


def exact_mean(occs):
    """float32(exact_sum / count) over occs >= 0 (all levels); NaN for an empty selection.  The sum is exact (math.fsum: the correctly
    rounded double of the true sum, the true sum itself whenever that is a double), the division is one double division."""
    occs = np.asarray(occs, np.float32).reshape(-1)
    with np.errstate(invalid="ignore"):
        sel = occs[occs >= 0]
    if sel.shape[0] == 0:
        return np.float32(np.nan)
    return np.float32(math.fsum(sel.astype(np.float64).tolist()) / float(sel.shape[0]))


def binarize(occs, cells, levels, occ_thre):
    """occ_grid.py:436-437 -> (binaries u8 [L,cells], bits u32 [L,words], thre f32): thre = min(mean(occs[occs >= 0]), occ_thre) over all
    levels, NaN if no cell qualifies (then nothing is occupied); binaries = occs > thre, strictly."""
    occs = np.asarray(occs, np.float32).reshape(-1)
    assert occs.shape[0] == cells * levels
    thre = exact_mean(occs)
    if not np.isnan(thre):
        thre = min(thre, np.float32(occ_thre))
    return binarize_at(occs, cells, levels, thre) + (np.float32(thre),)


def binarize_at(occs, cells, levels, thre):
    """(binaries u8 [L,cells], bits u32 [L,words]) of a given threshold"""
    with np.errstate(invalid="ignore"):
        binaries = (np.asarray(occs, np.float32).reshape(levels, cells) > np.float32(thre)).astype(np.uint8)
    return binaries, pack_bits(binaries)


def update(occs, binaries, res, aabbs, step, warmup_steps, seed, occ_eval_fn, occ_thre=0.01, ema_decay=0.95, value_scale=1.0):
    """One `_update` of L levels: occs [L*cells] f32, binaries [L,cells] (the state BEFORE the refresh: the occupied half reads it),
    aabbs [L,6]; level l draws with seed + l.  occ_eval_fn(points f32 [cap,3]) -> [cap] f32.
    -> (occs, binaries u8 [L,cells], bits u32 [L,words], thre, lists), lists = the (idx, pts) of every level."""
    cells = int(np.prod([int(r) for r in res]))
    aabbs = np.asarray(aabbs, np.float32).reshape(-1, 6)
    levels = aabbs.shape[0]
    occs = np.asarray(occs, np.float32).reshape(levels, cells).copy()
    binaries = np.asarray(binaries).reshape(levels, cells)
    lists = []
    for lvl in range(levels):
        idx, pts = sample_list(occs[lvl], binaries[lvl], res, aabbs[lvl], step, warmup_steps, int(seed) + lvl)
        vals = np.asarray(occ_eval_fn(pts), np.float32).reshape(-1) if idx.shape[0] else np.zeros(0, np.float32)
        occs[lvl] = apply(occs[lvl], idx, vals, value_scale, ema_decay)
        lists.append((idx, pts))
    new_bin, bits, thre = binarize(occs.reshape(-1), cells, levels, occ_thre)
    return occs.reshape(-1), new_bin, bits, thre, lists
