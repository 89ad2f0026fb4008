"""-m gpu: the rulebook kernels alone (csrc/rulebook.hip) against the brute-force references of tests/rulebook_cases.py, EXACTLY,
on the grids KITTI never shows them: widths that are no multiple of a bitmap word, odd depths, voxels on every grid face, grids
smaller than a word and fully occupied ones, the block / super-counter / scan-round boundaries of the counters, keys above 2^31,
truncated levels, a hash chain across the end of its table, and the ordered compaction of sassd_rulebook_pairs at all 27 offsets.
The per-op chain (sassd/spconv.py, selectable in FramePlan) and the fused pyramid (inference and training) in its three forms."""
import numpy as np
import pytest
import torch

from sassd import kernels as K, _C
import rulebook_cases as RC

pytestmark = pytest.mark.gpu

I32 = torch.int32
# Poison of the output buffers.  Tables and counts start negative (every consumer reads a negative entry as "no row" / "no rows").
# Coordinates start at the valid cell (0, 0, 0, 0), as in test_rulebook_pyramid_bit_exact: the phase behind an emit trusts the rows
# below the count, so a kernel that counted a row it never wrote would use a negative poison as an ADDRESS on the GPU instead of
# failing the comparison here.
TABLE_POISON, COUNT_POISON, COORD_POISON = -5, -7, 0


def _dev(a, dev, dtype=I32):
    return torch.tensor(np.asarray(a), dtype=dtype, device=dev)          # (a copy: the shared references stay unchanged)


def _np(t):
    return t.cpu().numpy()


def _check_pairs(pairs, num, table, n):
    """spconv-format pairs of the first n rows of `table` (numpy): all 27 offsets, order included, -1 past the count."""
    rp, rnum = RC.ref_pairs(table, n)
    pc, nc = _np(pairs), _np(num)
    assert np.array_equal(nc, rnum)
    for k in range(27):
        m = int(rnum[k])
        assert np.array_equal(pc[k, 0, :m], rp[k][0]) and np.array_equal(pc[k, 1, :m], rp[k][1]), "offset %d" % k
        assert np.all(pc[k, :, m:] == -1), "offset %d: entries past pair_num written" % k


def _level0_buffer(dev, c, rows):
    """[rows, 4] device coordinates: the case's rows, then valid-looking spare rows."""
    n0 = len(c["idx"])
    buf = np.concatenate([c["idx"], RC.spare_rows(np.random.default_rng(9), max(rows - n0, 0), c["batch"], c["shape"])], 0)
    return _dev(buf, dev)


def _run_chain(dev, name, caps, ref, levels, expect_status):
    """HashTable.build -> rulebook_subm -> rulebook_pairs -> rulebook_conv level after level, each level fed the device's own
    output after it was found equal to the reference.  caps[l]: the capacity the kernels are told for level l."""
    c = RC.CASE[name]
    batch, shape = c["batch"], c["shape"]
    n0 = len(c["idx"])
    st = K.new_status(dev)
    cap = caps[0]
    di = _level0_buffer(dev, c, max(cap, n0, 1))
    nptr = torch.tensor([n0], dtype=I32, device=dev)
    for l in range(levels):
        lv = ref[l]
        n = len(lv["idx"])
        assert cap >= max(n, 1)
        spare = di.clone()
        tab = K.HashTable(cap, dev).build(di, nptr, shape, batch, st)
        nbr = torch.full((cap, 27), TABLE_POISON, dtype=I32, device=dev)
        K.rulebook_subm(di, nptr, cap, shape, batch, tab, nbr=nbr)
        assert torch.equal(di, spare), "coordinates written by a table kernel"
        got = _np(nbr)
        assert np.array_equal(got[:n], lv["subm"]), "%s: subm level %d" % (name, l)
        assert np.all(got[n:] == TABLE_POISON), "%s: subm level %d rows past the count written" % (name, l)
        _check_pairs(*K.rulebook_pairs(nbr, nptr, cap), lv["subm"], n)
        if l + 1 == levels:
            break
        nx = ref[l + 1]
        m_ref, cap_out = len(nx["idx"]), caps[l + 1]
        oi = _dev(RC.spare_rows(np.random.default_rng(l), cap_out, batch, nx["shape"]), dev)
        oi0 = oi.clone()
        on = torch.tensor([COUNT_POISON], dtype=I32, device=dev)
        onb = torch.full((cap_out, 27), TABLE_POISON, dtype=I32, device=dev)
        K.rulebook_conv(di, nptr, cap, shape, batch, tab, cap_out, out_indices=oi, n_out_ptr=on, nbr=onb, status=st)
        m = int(on.item())
        assert m == m_ref, "%s: level %d has %d rows, reference %d" % (name, l + 1, m, m_ref)
        assert np.array_equal(_np(oi[:m]), nx["idx"]), "%s: coordinates level %d" % (name, l + 1)
        assert torch.equal(oi[m:], oi0[m:]), "%s: coordinates past the count written" % name
        got = _np(onb)
        assert np.array_equal(got[:m], nx["down"]), "%s: strided table into level %d" % (name, l + 1)
        assert np.all(got[m:] == TABLE_POISON)
        _check_pairs(*K.rulebook_pairs(onb, on, cap_out), nx["down"], m)
        di, nptr, cap, shape = oi, on, cap_out, nx["shape"]
    assert int(st.item()) == expect_status, "status 0x%x" % int(st.item())


@pytest.mark.parametrize("spare", [0, 37])
@pytest.mark.parametrize("name", RC.CHAIN_CASES)
def test_chain(dev, name, spare):
    """cap == n and cap = n + 37 with poisoned but valid-looking spare rows."""
    ref = RC.reference(name)
    try:
        _run_chain(dev, name, [max(len(lv["idx"]) + spare, 1) for lv in ref], ref, RC.chain_levels(name), 0)
    finally:
        if name == "rounds":                       # its 61 MB bitmap does not stay in the grow-only workspace cache
            for key in [k for k in K._ws_cache if k[0] == "rulebook_conv"]:
                del K._ws_cache[key]


def _run_pyramid(dev, name, form, caps, ref, expect_status):
    """RulebookPyramid whole (in launches), staged level by level, or persistent; twice, so that the workspace reset is checked.
    Counts of the levels >= 1 start at COUNT_POISON, tables at TABLE_POISON, coordinates at COORD_POISON."""
    c = RC.CASE[name]
    levels, n0 = c["levels"], len(c["idx"])
    idx = [_level0_buffer(dev, c, max(caps[0], n0, 1))] + \
          [torch.full((cp, 4), COORD_POISON, dtype=I32, device=dev) for cp in caps[1:]]
    idx0 = idx[0].clone()
    n = [torch.tensor([n0 if l == 0 else COUNT_POISON], dtype=I32, device=dev) for l in range(levels)]
    subm = [torch.full((cp, 27), TABLE_POISON, dtype=I32, device=dev) for cp in caps]
    down = [None] + [torch.full((cp, 27), TABLE_POISON, dtype=I32, device=dev) for cp in caps[1:]]
    st = K.new_status(dev)
    pyr = K.RulebookPyramid(idx, n, caps, c["shape"], c["batch"], subm, down, st)
    for rep in range(2):
        if form == "staged":
            for l in range(levels):
                pyr.build(l, l + 1)
        else:
            pyr.build(persistent=(form == "persistent"))
        torch.cuda.synchronize()
        assert int(st.item()) == expect_status, "%s %s: status 0x%x (build %d)" % (name, form, int(st.item()), rep)
        assert torch.equal(idx[0], idx0) and int(n[0].item()) == n0, "level-0 input written"
        for l, lv in enumerate(ref):
            m = len(lv["idx"])
            if l:
                assert int(n[l].item()) == m, "%s %s: level %d has %d rows, reference %d" % (name, form, l, int(n[l].item()), m)
                got = _np(idx[l])
                assert np.array_equal(got[:m], lv["idx"]), "%s %s: coordinates level %d" % (name, form, l)
                assert np.all(got[m:] == COORD_POISON), "%s %s: coordinates past the count written" % (name, form)
                got = _np(down[l])
                assert np.array_equal(got[:m], lv["down"]), "%s %s: strided table into level %d" % (name, form, l)
                assert np.all(got[m:] == TABLE_POISON)
            got = _np(subm[l])
            assert np.array_equal(got[:m], lv["subm"]), "%s %s: subm level %d" % (name, form, l)
            assert np.all(got[m:] == TABLE_POISON), "%s %s: subm level %d rows past the count written" % (name, form, l)
        for l in range(1, levels):                 # the second build starts from poison again
            idx[l].fill_(COORD_POISON)
            subm[l].fill_(TABLE_POISON)
            down[l].fill_(TABLE_POISON)
            n[l].fill_(COUNT_POISON)
        subm[0].fill_(TABLE_POISON)
    del pyr
    if name == "high-key":
        torch.cuda.empty_cache()                   # (a 340 MB workspace)


@pytest.mark.parametrize("form", ["whole", "staged"])
@pytest.mark.parametrize("name", RC.PYRAMID_CASES)
def test_pyramid(dev, name, form):
    ref = RC.reference(name)
    _run_pyramid(dev, name, form, [max(len(lv["idx"]) + 11, 1) for lv in ref], ref, 0)


@pytest.mark.parametrize("name", RC.PERSISTENT_CASES)
def test_pyramid_persistent(dev, name):
    """One launch, phases separated by grid barriers; the spin is bounded and sets a status bit: status stays 0."""
    ref = RC.reference(name)
    _run_pyramid(dev, name, "persistent", [max(len(lv["idx"]) + 11, 1) for lv in ref], ref, 0)


@pytest.mark.parametrize("name,level", RC.TRUNCATED)
def test_truncated_levels(dev, name, level):
    """A level that cannot hold its rows keeps the first cap of them in ascending order with unchanged strided tables, its
    submanifold table has no neighbour at or past cap, the next level is built from the truncated set; status has exactly the
    VOXEL_OVERFLOW bit.  Level-0 rows past caps[0] do not exist (no flag: the voxelizer raises its own)."""
    caps, ref = RC.truncated_caps(name, level)
    status = _C.ST_VOXEL_OVERFLOW if level else 0
    assert RC.ST_VOXEL_OVERFLOW == _C.ST_VOXEL_OVERFLOW
    assert len(ref[level]["idx"]) == caps[level]
    _run_chain(dev, name, caps, ref, len(ref), status)
    for form in ("whole", "staged"):
        _run_pyramid(dev, name, form, caps, ref, status)


@pytest.mark.parametrize("n", RC.PAIRS_ROWS)
def test_pairs_alone(dev, n):
    """The 1024-row rounds of pairs_kernel: ordered compaction, an offset without a pair, one where every row has a pair, cap > n
    with live-looking rows past n."""
    nbr, cap = RC.pairs_case(n)
    pairs, num = K.rulebook_pairs(_dev(nbr, dev), torch.tensor([n], dtype=I32, device=dev), cap)
    _check_pairs(pairs, num, nbr, n)
    assert int(num[RC.PAIRS_EMPTY_K].item()) == 0 and int(num[RC.PAIRS_FULL_K].item()) == n


def test_hash_probes_across_the_table_end(dev):
    """40 keys whose home slot is one of the last three of a 1024-slot table: the table itself is read back and held to what the
    case claims (if the hash ever changes this fails loudly, the case does not silently lose its point), then the tables, which
    include lookups of absent neighbours that walk the chain across the end to an empty slot; the same rows as level 0 of a
    pyramid with caps[0] = 300."""
    hc = RC.hash_wrap_case()
    idx, mask = hc["idx"], hc["mask"]
    n, cap, batch, shape = len(idx), RC.HASH_CAP, RC.HASH_BATCH, RC.HASH_SHAPE
    ref = RC.ref_pyramid(idx, shape, 2)
    buf = np.concatenate([idx, RC.spare_rows(np.random.default_rng(4), cap - n, batch, shape)], 0)
    di = _dev(buf, dev)
    nptr = torch.tensor([n], dtype=I32, device=dev)
    st = K.new_status(dev)
    tab = K.HashTable(cap, dev).build(di, nptr, shape, batch, st)
    assert tab.nbytes == 8 * (mask + 1)
    ent = _np(tab.buf.view(I32)).view(np.uint32).reshape(-1, 2)
    RC.check_hash_table(ent, RC.lin(idx, shape), mask)
    nbr = torch.full((cap, 27), TABLE_POISON, dtype=I32, device=dev)
    K.rulebook_subm(di, nptr, cap, shape, batch, tab, nbr=nbr)
    assert np.array_equal(_np(nbr[:n]), ref[0]["subm"]) and bool((nbr[n:] == TABLE_POISON).all())
    m = len(ref[1]["idx"])
    oi, on, onb = K.rulebook_conv(di, nptr, cap, shape, batch, tab, m + 3, status=st)
    assert int(on.item()) == m and int(st.item()) == 0
    assert np.array_equal(_np(oi[:m]), ref[1]["idx"]) and np.array_equal(_np(onb[:m]), ref[1]["down"])
    # level 0 of a pyramid: the same hash inside the fused form
    caps = [cap, m + 3]
    idxs = [di, torch.full((caps[1], 4), COORD_POISON, dtype=I32, device=dev)]
    ns = [nptr, torch.tensor([COUNT_POISON], dtype=I32, device=dev)]
    subm = [torch.full((cp, 27), TABLE_POISON, dtype=I32, device=dev) for cp in caps]
    down = [None, torch.full((caps[1], 27), TABLE_POISON, dtype=I32, device=dev)]
    K.RulebookPyramid(idxs, ns, caps, shape, batch, subm, down, st).build()
    torch.cuda.synchronize()
    assert int(st.item()) == 0 and int(ns[1].item()) == m
    assert np.array_equal(_np(subm[0][:n]), ref[0]["subm"]) and bool((subm[0][n:] == TABLE_POISON).all())
    assert np.array_equal(_np(idxs[1][:m]), ref[1]["idx"]) and np.array_equal(_np(down[1][:m]), ref[1]["down"])
    assert np.array_equal(_np(subm[1][:m]), ref[1]["subm"])
