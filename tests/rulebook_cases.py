"""References and seeded cases of the kernel-level tests of the sparse front end (test_rulebook_cases_cpu.py,
test_gpu_rulebook_kernels.py, test_gpu_densify_kernels.py): numpy only, nothing here touches a GPU.

Every kernel under test produces integers or copies, so every comparison is EXACT: there is no tolerance anywhere.

A. rulebook references (csrc/rulebook.hip: the per-op chain sassd_hash_build / _rulebook_subm / _rulebook_conv / _rulebook_pairs
   and the fused sassd_rulebook_pyramid in its three forms)
------------------------------------------------------------------------------------------------------------------------------
ref_subm / ref_down are brute force over a Python dict keyed by (b, z, y, x), written independently of oracle/rulebook.py (no
searchsorted, no linear keys); test_rulebook_cases_cpu.py proves them equal to it on every untruncated case and to the nonzero
set of F.conv3d(occupancy, ones(3, 3, 3), stride 2, padding 1) on the grids under 1e5 cells.
  offset           k = (kz * 3 + ky) * 3 + kx
  submanifold      the neighbour of row r at offset k is the voxel at c + (k - 1) per axis, or -1
  strided k3 s2 p1 output shape (s - 1) // 2 + 1 per axis, outputs ascending in (b, z, y, x), nbr[o, k] = the input row at
                   2 * o - 1 + kk per axis
  truncation       (as the kernels implement it) with cap_out the output set keeps its first cap_out rows in ascending order and
                   their strided tables unchanged; the submanifold table of the truncated level maps neighbours whose row is
                   >= cap to -1 (= ref_subm of the truncated set); the next level is built from the truncated set; level-0
                   rows past caps[0] do not exist
  ref_pairs        per offset the (in_row, out_row) pairs in ascending out-row order, and the counts

B. grids (level-0 rows in a seeded random order, never sorted)
------------------------------------------------------------------------------------------------------------------------------
  case         batch, shape            occupancy        why
  one          1, (1, 1, 1)            full             smallest pyramid: every level is (1, 1, 1)
  three        3, (1, 1, 1)            full             three batches in one bitmap word
  dense-small  3, (3, 5, 7)            full             W < 32, batch boundary mid-word, all 27 neighbours live
  odd-31       2, (2, 33, 31)          50 %             W one short of a word
  odd-65       2, (5, 9, 65)           30 %             W two words + 1
  dense-33     3, (7, 6, 33)           full             every word full: carries on every bit
  deep-41      2, (41, 17, 95)         2 %              a 41-deep grid, odd at every level (41 -> 21 -> 11 -> 6)
  column       2, (1, 64, 1)           70 %             two degenerate axes
  corners      2, (6, 10, 34)          8 corners of each batch + 1 centre: every face test of axis_outs and of the bounds checks
  empty        1, (3, 5, 7)            n = 0            no row anywhere, status stays 0
  counters     1, (8, 800, 1400)       2 x the coordinates of the level-1 cells 0, 31, 32, 8191, 8192, 524287, 524288, 1048575,
                                       1048576, 1119999 + 300 random: level 1 is (4, 400, 700) = 35 000 words = 137 blocks of the
                                       pyramid = two full 64-block super-counters + 9; W = 700 is no multiple of 32
  rounds       2, (40, 7000, 7000)     chain only: 490 000 000 output cells = 14 954 blocks of 1024 words = 15 rounds of
                                       blocksum_scan_kernel, keys up to 3 919 999 999 > 2^31; 2 x the output cells
                                       32768 * 1024 - 1, 32768 * 1024, 32768 * 2048 - 1, 32768 * 2048 and the last, the 16 corners,
                                       600 random
  high-key     2, (4, 16400, 16400)    pyramid only, 2 levels: 2 151 680 000 level-0 cells, hash keys cross 2^31; the 16
                                       corners, 300 random, 4 voxels whose key is within 3 of the largest
Truncated runs: dense-small and odd-65 with 60 % of the reference's rows at level 1 (one run) and at level 2 (another);
caps[0] below n0 on odd-31.

C. hash wrap: batch 2, (8, 64, 96), capacity 300 -> 1024 slots, mask 1023.  hash_u32 is restated here; 40 voxels whose home slot is
   >= 1021 (279 such cells exist) + 20 face neighbours of those.  Linear probing makes the SET of occupied slots independent of the
   insertion order: the chain from slot 1021 runs across the end of the table into slots 0.. .

D. pairs alone: synthetic tables of n in {0, 1, 1023, 1024, 1025, 2049} rows (the 1024-row rounds of pairs_kernel), one offset
   without a pair and one where every row has a pair, live-looking rows past n.

E. densify family and voxel mean: see densify_cases / bf16_patterns / voxel_mean_case and the integer rounding rule round_bf16_bits.
"""
import numpy as np

I32 = np.int32
EMPTY_KEY = 0xFFFFFFFF
ST_VOXEL_OVERFLOW = 1


# ---- A. references ---------------------------------------------------------------------------------------------------------
def out_shape(shape):
    return tuple((int(s) - 1) // 2 + 1 for s in shape)


def ref_subm(idx, shape):
    """[n, 27] table: row of the voxel at c + (k - 1) per axis, or -1 (cells outside the grid hold no voxel)."""
    rows = [tuple(c) for c in np.asarray(idx).reshape(-1, 4).tolist()]
    at = {c: r for r, c in enumerate(rows)}
    assert len(at) == len(rows), "duplicate coordinates"
    nbr = np.full((len(rows), 27), -1, I32)
    for r, (b, z, y, x) in enumerate(rows):
        for kz in range(3):
            for ky in range(3):
                for kx in range(3):
                    nbr[r, (kz * 3 + ky) * 3 + kx] = at.get((b, z + kz - 1, y + ky - 1, x + kx - 1), -1)
    return nbr


def ref_down(idx, shape, cap_out=None):
    """(out_idx [m, 4], nbr [m, 27], out shape, untruncated row count) of SparseConv3d(k3, s2, p1)."""
    rows = [tuple(c) for c in np.asarray(idx).reshape(-1, 4).tolist()]
    at = {c: r for r, c in enumerate(rows)}
    oshape = out_shape(shape)

    def outs(i, od):            # outputs o with 2 o - 1 + kk == i for some kk in {0, 1, 2}
        return [o for o in ((i + 1) // 2, i // 2) if 0 <= o < od and 0 <= i - (2 * o - 1) <= 2]
    active = set()
    for (b, z, y, x) in rows:
        for oz in outs(z, oshape[0]):
            for oy in outs(y, oshape[1]):
                for ox in outs(x, oshape[2]):
                    active.add((b, oz, oy, ox))
    out = sorted(active)
    total = len(out)
    if cap_out is not None:
        out = out[:cap_out]
    nbr = np.full((len(out), 27), -1, I32)
    for o, (b, z, y, x) in enumerate(out):
        for kz in range(3):
            for ky in range(3):
                for kx in range(3):
                    nbr[o, (kz * 3 + ky) * 3 + kx] = at.get((b, 2 * z - 1 + kz, 2 * y - 1 + ky, 2 * x - 1 + kx), -1)
    return np.array(out, I32).reshape(-1, 4), nbr, oshape, total


def ref_pyramid(idx0, shape, levels, caps=None):
    """Per level dict(idx, shape, subm, down (None at level 0), total = the untruncated row count of the level)."""
    idx0 = np.asarray(idx0, I32).reshape(-1, 4)
    total = len(idx0)
    if caps is not None:
        idx0 = idx0[:caps[0]]
    out = [dict(idx=idx0, shape=tuple(shape), subm=ref_subm(idx0, shape), down=None, total=total)]
    for l in range(1, levels):
        p = out[-1]
        oi, nbr, osh, total = ref_down(p["idx"], p["shape"], None if caps is None else caps[l])
        out.append(dict(idx=oi, shape=osh, subm=ref_subm(oi, osh), down=nbr, total=total))
    return out


def ref_pairs(nbr, n):
    """([(in_rows, out_rows)] * K in ascending out-row order, counts [K]) of the first n rows of a gather table."""
    nbr = np.asarray(nbr)
    pairs, num = [], np.zeros(nbr.shape[1], I32)
    for k in range(nbr.shape[1]):
        ins, outs = [], []
        for r in range(n):
            if nbr[r, k] >= 0:
                ins.append(int(nbr[r, k]))
                outs.append(r)
        pairs.append((np.array(ins, I32), np.array(outs, I32)))
        num[k] = len(outs)
    return pairs, num


# ---- B. grids --------------------------------------------------------------------------------------------------------------
def unlin(cells, batch, shape):
    """[n, 4] (b, z, y, x) of linear cell numbers of a (batch, *shape) grid."""
    c = np.asarray(cells, np.int64)
    d, h, w = shape
    assert np.all((c >= 0) & (c < batch * d * h * w))
    return np.stack([c // (d * h * w), (c // (h * w)) % d, (c // w) % h, c % w], 1)


def lin(idx, shape):
    i = np.asarray(idx, np.int64).reshape(-1, 4)
    d, h, w = shape
    return ((i[:, 0] * d + i[:, 1]) * h + i[:, 2]) * w + i[:, 3]


def corners(batch, shape):
    d, h, w = shape
    return np.array([(b, z, y, x) for b in range(batch) for z in (0, d - 1) for y in (0, h - 1) for x in (0, w - 1)], np.int64)


def _finish(rng, parts, batch, shape):
    """Unique rows of `parts` in a seeded random order."""
    cells = np.unique(lin(np.concatenate(parts, 0), shape))
    idx = unlin(cells, batch, shape)
    return np.ascontiguousarray(idx[rng.permutation(len(idx))], I32)


def _random_cells(rng, count, batch, shape):
    d, h, w = shape
    return np.stack([rng.integers(0, batch, count), rng.integers(0, d, count), rng.integers(0, h, count),
                     rng.integers(0, w, count)], 1).astype(np.int64)


def _fraction(rng, frac, batch, shape):
    cells = batch * int(np.prod(shape))
    pick = rng.permutation(cells)[:int(round(frac * cells))]
    return np.ascontiguousarray(unlin(pick, batch, shape), I32)          # (a permutation's prefix: already in random order)


COUNTERS_CELLS = (0, 31, 32, 8191, 8192, 524287, 524288, 1048575, 1048576, 1119999)
ROUNDS_CELLS = (32768 * 1024 - 1, 32768 * 1024, 32768 * 2048 - 1, 32768 * 2048, 490000000 - 1)


def _twice(cells, batch, shape1):
    c = unlin(cells, batch, shape1)
    c[:, 1:] *= 2                                                      # an all-even input coordinate reaches exactly one output
    return c


def _case(name, batch, shape, idx, levels=4, chain=True, pyramid=True, persistent=False, **claims):
    return dict(name=name, batch=batch, shape=tuple(shape), idx=np.ascontiguousarray(idx, I32).reshape(-1, 4), levels=levels,
                chain=chain, pyramid=pyramid, persistent=persistent, claims=claims)


def _build_cases():
    rng = np.random.default_rng(20240611)
    cs = []
    cs.append(_case("one", 1, (1, 1, 1), _fraction(rng, 1.0, 1, (1, 1, 1)), persistent=True))
    cs.append(_case("three", 3, (1, 1, 1), _fraction(rng, 1.0, 3, (1, 1, 1)), word_spans_batches=True))
    cs.append(_case("dense-small", 3, (3, 5, 7), _fraction(rng, 1.0, 3, (3, 5, 7)), persistent=True, word_spans_batches=True,
                    word_spans_rows=True, full_neighbourhood=True))
    cs.append(_case("odd-31", 2, (2, 33, 31), _fraction(rng, 0.5, 2, (2, 33, 31)), word_spans_rows=True))
    cs.append(_case("odd-65", 2, (5, 9, 65), _fraction(rng, 0.3, 2, (5, 9, 65)), persistent=True, word_spans_rows=True))
    cs.append(_case("dense-33", 3, (7, 6, 33), _fraction(rng, 1.0, 3, (7, 6, 33)), word_spans_rows=True, word_spans_batches=True,
                    full_words=True))
    cs.append(_case("deep-41", 2, (41, 17, 95), _fraction(rng, 0.02, 2, (41, 17, 95)), word_spans_rows=True,
                    shapes=((41, 17, 95), (21, 9, 48), (11, 5, 24), (6, 3, 12))))
    cs.append(_case("column", 2, (1, 64, 1), _fraction(rng, 0.7, 2, (1, 64, 1)), word_spans_rows=True))
    sh = (6, 10, 34)
    cs.append(_case("corners", 2, sh, _finish(rng, [corners(2, sh), np.array([(0, 3, 5, 17), (1, 3, 5, 17)])], 2, sh),
                    cells0=tuple(int(v) for v in lin(corners(2, sh), sh))))
    cs.append(_case("empty", 1, (3, 5, 7), np.zeros((0, 4), I32)))
    sh = (8, 800, 1400)
    cs.append(_case("counters", 1, sh, _finish(rng, [_twice(COUNTERS_CELLS, 1, out_shape(sh)), _random_cells(rng, 300, 1, sh)],
                                               1, sh), persistent=True, cells1=COUNTERS_CELLS))
    sh = (40, 7000, 7000)
    cs.append(_case("rounds", 2, sh, _finish(rng, [_twice(ROUNDS_CELLS, 2, out_shape(sh)), corners(2, sh),
                                                   _random_cells(rng, 600, 2, sh)], 2, sh), pyramid=False,
                    cells1=ROUNDS_CELLS, cells0=tuple(int(v) for v in lin(corners(2, sh), sh)), key_above_2_31=True))
    sh = (4, 16400, 16400)
    top = 2 * 4 * 16400 * 16400 - 1
    cs.append(_case("high-key", 2, sh, _finish(rng, [corners(2, sh), _random_cells(rng, 300, 2, sh),
                                                     unlin([top - 3, top - 2, top - 1, top], 2, sh)], 2, sh), levels=2,
                    chain=False, cells0=tuple(int(v) for v in lin(corners(2, sh), sh)) + (top - 3, top - 2, top - 1, top),
                    key_above_2_31=True))
    return cs


CASES = _build_cases()
CASE = {c["name"]: c for c in CASES}
CHAIN_CASES = [c["name"] for c in CASES if c["chain"]]
PYRAMID_CASES = [c["name"] for c in CASES if c["pyramid"]]
PERSISTENT_CASES = [c["name"] for c in CASES if c["persistent"]]
# (case, level whose capacity is 60 % of the reference's rows); level 0: caps[0] below n0
TRUNCATED = [("dense-small", 1), ("dense-small", 2), ("odd-65", 1), ("odd-65", 2), ("odd-31", 0)]

_ref_cache = {}


def reference(name):
    """The untruncated reference pyramid of a case, computed once and shared (callers must not write into it)."""
    if name not in _ref_cache:
        c = CASE[name]
        ref = ref_pyramid(c["idx"], c["shape"], c["levels"])
        for lv in ref:
            for a in (lv["idx"], lv["subm"], lv["down"]):
                if a is not None:
                    a.setflags(write=False)
        _ref_cache[name] = ref
    return _ref_cache[name]


def chain_levels(name):
    """Levels of the per-op chain: 4, or up to the first level of shape (1, 1, 1) that a strided conv produced."""
    ref = reference(name)
    n = 1
    while n < len(ref) and not (n > 1 and ref[n - 1]["shape"] == (1, 1, 1)):
        n += 1
    return n


def truncated_caps(name, level):
    """Capacities of a truncated run: 60 % of the reference's rows at `level`, the (then smaller) exact counts elsewhere + 5."""
    c = CASE[name]
    full = reference(name)
    caps = [len(lv["idx"]) + 5 for lv in full]
    caps[level] = (6 * len(full[level]["idx"])) // 10
    ref = ref_pyramid(c["idx"], c["shape"], c["levels"], caps)
    return caps, ref


def spare_rows(rng, count, batch, shape):
    """Valid-looking coordinates for buffer rows past the row count (a kernel that read them would build tables from them)."""
    return np.ascontiguousarray(_random_cells(rng, count, batch, shape), I32)


def words_spanning(idx, shape, axis):
    """Number of 32-cell bitmap words of the (batch, *shape) grid holding occupied cells that differ in column `axis` of idx."""
    idx = np.asarray(idx).reshape(-1, 4)
    if len(idx) == 0:
        return 0
    word = lin(idx, shape) >> 5
    order = np.argsort(word, kind="stable")
    w, v = word[order], idx[order, axis]
    same = w[1:] == w[:-1]
    return int(np.unique(w[1:][same & (v[1:] != v[:-1])]).size)


# ---- C. hash wrap ----------------------------------------------------------------------------------------------------------
def hash_u32(k):
    k = np.array(k, np.uint64) & np.uint64(0xFFFFFFFF)
    k ^= k >> 16
    k = (k * 0x7feb352d) & 0xFFFFFFFF
    k ^= k >> 15
    k = (k * 0x846ca68b) & 0xFFFFFFFF
    k ^= k >> 16
    return k.astype(np.uint32)


def hash_slots(cap_rows):
    h = 1
    while h < 2 * max(int(cap_rows), 1):
        h *= 2
    return max(h, 1024)


HASH_BATCH, HASH_SHAPE, HASH_CAP, HASH_HOME = 2, (8, 64, 96), 300, 1021


def hash_wrap_case():
    """dict(idx [60, 4] in random order, homes = number of cells whose home slot is >= HASH_HOME, mask)."""
    rng = np.random.default_rng(77)
    mask = hash_slots(HASH_CAP) - 1
    cells = np.arange(HASH_BATCH * int(np.prod(HASH_SHAPE)), dtype=np.int64)
    home = hash_u32(cells) & mask
    late = cells[home >= HASH_HOME]
    chain = unlin(late[rng.permutation(len(late))[:40]], HASH_BATCH, HASH_SHAPE)
    taken = {tuple(c) for c in chain.tolist()}
    extra = []
    d, h, w = HASH_SHAPE
    steps = [(0, 1, 0, 0), (0, -1, 0, 0), (0, 0, 1, 0), (0, 0, -1, 0), (0, 0, 0, 1), (0, 0, 0, -1)]
    for c in chain.tolist():
        if len(extra) == 20:
            break
        for s in (steps[i] for i in rng.permutation(6)):
            q = tuple(int(a + b) for a, b in zip(c, s))
            if 0 <= q[1] < d and 0 <= q[2] < h and 0 <= q[3] < w and q not in taken:
                taken.add(q)
                extra.append(q)
                break
    idx = np.concatenate([chain, np.array(extra, np.int64)], 0)
    return dict(idx=np.ascontiguousarray(idx[rng.permutation(len(idx))], I32), homes=int(len(late)), mask=mask)


def hash_insert_all(keys, mask):
    """Linear-probing table after inserting `keys` (in this order; the occupied SET does not depend on it): keys per slot."""
    slots = np.full(mask + 1, EMPTY_KEY, np.uint64)
    for k in np.asarray(keys, np.uint64).tolist():
        h = int(hash_u32(k)) & mask
        while slots[h] != EMPTY_KEY and slots[h] != k:
            h = (h + 1) & mask
        slots[h] = k
    return slots


def check_hash_table(ent, keys, mask):
    """Asserts what the hash case claims of a table ([slots, 2] {key, row}): slots mask and 0 hold keys whose home is >= HASH_HOME;
    every key sits at or after its home with no empty slot in between, and carries its row; nothing else is in the table."""
    ent = np.asarray(ent, np.uint64).reshape(-1, 2)
    assert len(ent) == mask + 1
    for s in (mask, 0):
        assert ent[s, 0] != EMPTY_KEY, "slot %d is empty: the chain does not cross the end of the table" % s
        assert (int(hash_u32(ent[s, 0])) & mask) >= HASH_HOME, "slot %d holds a key whose home is not at the table's end" % s
    for row, k in enumerate(np.asarray(keys, np.uint64).tolist()):
        h = int(hash_u32(k)) & mask
        probes = 0
        while ent[h, 0] != k:
            assert ent[h, 0] != EMPTY_KEY, "key %d: an empty slot between its home and itself (or not inserted)" % k
            h = (h + 1) & mask
            probes += 1
            assert probes <= mask
        assert ent[h, 1] == row, "key %d carries row %d, not %d" % (k, ent[h, 1], row)
    assert int((ent[:, 0] != EMPTY_KEY).sum()) == len(keys)


# ---- D. pairs alone --------------------------------------------------------------------------------------------------------
PAIRS_ROWS = (0, 1, 1023, 1024, 1025, 2049)
PAIRS_EMPTY_K, PAIRS_FULL_K = 5, 20


def pairs_case(n):
    """(nbr [cap, 27], cap): random table, offset PAIRS_EMPTY_K without a pair, PAIRS_FULL_K with one in every row, rows past n
    holding live-looking entries."""
    rng = np.random.default_rng(1000 + n)
    cap = n + 19
    nbr = rng.integers(0, max(n, 1), (cap, 27)).astype(I32)
    nbr[rng.random((cap, 27)) < 0.5] = -1
    nbr[:, PAIRS_EMPTY_K] = -1
    nbr[:, PAIRS_FULL_K] = rng.integers(0, max(n, 1), cap)
    nbr[n:, PAIRS_EMPTY_K] = 0                                         # (past n even the empty offset looks alive)
    return nbr, cap


# ---- E. densify family and voxel mean --------------------------------------------------------------------------------------
SPECIAL_F32 = np.array([0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x807FFFFF, 0x7FC12345, 0x00000000, 0x3F800000],
                       np.uint32)      # -0.0, +inf, -inf, subnormals, a NaN with a payload, +0.0, 1.0

# (shape, batch, channels, row counts): n * C straddles 256 (the block size of the scatter kernels); 0 = empty
DENSIFY_F32 = [((3, 5, 7), 2, (3,), (0, 1, 85, 86)),              # 2520-byte map: not a multiple of 16 -> the memset branch
               ((5, 8, 16), 3, (1, 16, 64), None)]                # the fill-kernel branch
DENSIFY_BF16 = [((3, 4, 6), 2, (3,), (0, 1, 85, 86)),
                ((5, 8, 16), 3, (1, 16, 64), None)]


def densify_rows(c):
    return {1: (0, 255, 256, 257), 16: (0, 1, 16, 17), 64: (0, 3, 4, 5)}[c]


def densify_case(shape, batch, c, n, payload, seed=0):
    """dict(idx [cap, 4] distinct cells in random order, feats [cap, c] uint32 bit patterns, n, cap): rows past n carry valid
    coordinates (cells no live row uses) and non-zero features."""
    rng = np.random.default_rng(seed * 7919 + n * 131 + c)
    cap = n + 13
    cells = batch * int(np.prod(shape))
    assert cap <= cells
    idx = np.ascontiguousarray(unlin(rng.permutation(cells)[:cap], batch, shape), I32)
    bits = rng.integers(0, 1 << 32, (cap, c), dtype=np.uint64).astype(np.uint32)
    bits[(bits & 0x7F800000) == 0x7F800000] &= 0xBFFFFFFF              # random patterns: finite only
    flat = bits.reshape(-1)
    pos = rng.permutation(n * c)[:min(len(payload), n * c)]
    flat[pos] = payload[:len(pos)]
    bits[n:] |= 0x3F000000                                             # rows past n: never zero
    return dict(idx=idx, feats=bits, n=n, cap=cap)


def densify_ref_bits(idx, bits, n, shape, batch, order):
    """Scatter of the first n rows into a zero map [batch, C * D, H, W] (same dtype as bits): channel = c * D + z (order 0)
    or z * C + c (order 1)."""
    d, h, w = shape
    c = bits.shape[1]
    out = np.zeros((batch, c * d, h, w), bits.dtype)
    for r in range(n):
        b, z, y, x = (int(v) for v in idx[r])
        ch = np.arange(c) * d + z if order == 0 else z * c + np.arange(c)
        out[b, ch, y, x] = bits[r]
    return out


def bf16_patterns():
    """fp32 bit patterns at the edges of round-to-nearest-even into bf16."""
    p = []
    for hi in (0x3F80, 0x3F81, 0xC2FE, 0xC2FF, 0x0000, 0x0001, 0x8000, 0x7F7E, 0x007F, 0x0080):
        for lo in (0x8000, 0x7FFF, 0x8001, 0x0000, 0x0001, 0xFFFF):     # exact ties (even and odd upper half), one ulp either side
            p.append((hi << 16) | lo)
    p += [0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000, 0x7F7F7FFF,               # round to +-inf / stay finite
          0x00000001, 0x80000001, 0x00008000, 0x00007FFF, 0x00018000,  # subnormals
          0x00000000, 0x80000000, 0x7F800000, 0xFF800000,
          0x7FC00000, 0x7F800001, 0xFFC12345, 0x7F80FFFF]              # NaN (quiet, signalling, payload, payload below bit 16)
    return np.array(p, np.uint32)


def is_nan_bits32(u):
    u = np.asarray(u, np.uint32)
    return ((u & 0x7F800000) == 0x7F800000) & ((u & 0x007FFFFF) != 0)


def is_nan_bits16(u):
    u = np.asarray(u, np.uint16)
    return ((u & 0x7F80) == 0x7F80) & ((u & 0x007F) != 0)


def round_bf16_bits(u):
    """The integer rule of round-to-nearest-even, fp32 bits -> bf16 bits (valid for every non-NaN input)."""
    u = np.asarray(u, np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


VOXEL_MEAN_T = (1, 5, 8)
VOXEL_MEAN_DIMS = ((4, 4), (4, 3), (8, 8), (6, 3))
VOXEL_MEAN_M = (1, 64, 65, 1000)


def voxel_mean_case(m, t, ndim):
    """(voxels [m, t, ndim] fp32 with zero padding in the unused slots, num_points [m] in 1..t, every count present)."""
    rng = np.random.default_rng(m * 100 + t * 10 + ndim)
    num = rng.integers(1, t + 1, m).astype(I32)
    num[:min(m, t)] = np.arange(t, 0, -1)[:min(m, t)]
    v = (rng.standard_normal((m, t, ndim)) * np.array([30.0, 20.0, 2.0, 0.5] * 2)[:ndim]).astype(np.float32)
    v[np.arange(t)[None, :] >= num[:, None]] = 0.0
    return v, num


def voxel_mean_twin(voxels, num, nfeat):
    """fp32 twin of the kernel: slots 0 .. T - 1 added in order, one division."""
    s = np.zeros((voxels.shape[0], nfeat), np.float32)
    for t in range(voxels.shape[1]):
        s = (s + voxels[:, t, :nfeat]).astype(np.float32)
    return (s / num.astype(np.float32)[:, None]).astype(np.float32)
