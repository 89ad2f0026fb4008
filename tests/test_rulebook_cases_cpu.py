"""CPU proof of tests/rulebook_cases.py before any GPU is involved: the brute-force rulebook references equal oracle/rulebook.py
and F.conv3d's active set, every case fulfils the condition it exists for (recomputed from the case itself), the truncated cases
really overflow, the hash case really forms a chain across the end of its table, and the two statements of each densify /
bf16-rounding / voxel-mean reference agree with each other."""
import numpy as np
import pytest
import torch

from oracle import clib, nets as onets, rulebook as orb
import rulebook_cases as RC


@pytest.mark.parametrize("name", [c["name"] for c in RC.CASES])
def test_references_equal_the_oracle(name):
    c = RC.CASE[name]
    ref = RC.reference(name)
    assert len(ref) == c["levels"] and len(ref[0]["idx"]) == len(c["idx"])
    for l, lv in enumerate(ref):
        idx, shape = lv["idx"], lv["shape"]
        assert lv["total"] == len(idx)
        assert np.array_equal(orb.subm_rulebook(idx, shape)[1], lv["subm"]), (name, l)
        assert np.array_equal(lv["subm"][:, 13], np.arange(len(idx))), "the centre offset is the row itself"
        if l + 1 < len(ref):
            oi, nbr, oshape = orb.conv_rulebook(idx, shape, c["batch"])
            nx = ref[l + 1]
            assert tuple(oshape) == nx["shape"] == RC.out_shape(shape)
            assert np.array_equal(oi, nx["idx"]) and np.array_equal(nbr, nx["down"]), (name, l)
            if len(oi) > 1:
                k = RC.lin(oi, oshape)
                assert np.all(k[1:] > k[:-1]), "outputs ascend in (b, z, y, x)"
        for tab in (lv["subm"], lv["down"]):
            if tab is None or len(tab) > 5000:
                continue
            pairs, num = RC.ref_pairs(tab, len(tab))
            opairs, onum = orb.nbr_to_pairs(tab)
            assert np.array_equal(num, onum)
            for k in range(27):
                assert np.array_equal(pairs[k][0], opairs[k][0]) and np.array_equal(pairs[k][1], opairs[k][1])
    if name != "empty":
        assert all(len(lv["idx"]) > 0 for lv in ref)


@pytest.mark.parametrize("name", [c["name"] for c in RC.CASES if c["batch"] * int(np.prod(c["shape"])) < 100000])
def test_active_outputs_equal_conv3d(name):
    c = RC.CASE[name]
    ref = RC.reference(name)
    for l in range(len(ref) - 1):
        d, h, w = ref[l]["shape"]
        occ = torch.zeros(c["batch"], 1, d, h, w)
        i = torch.tensor(ref[l]["idx"], dtype=torch.int64).view(-1, 4)
        occ[i[:, 0], 0, i[:, 1], i[:, 2], i[:, 3]] = 1.0
        hit = torch.nn.functional.conv3d(occ, torch.ones(1, 1, 3, 3, 3), stride=2, padding=1)[:, 0]
        assert tuple(hit.shape[1:]) == ref[l + 1]["shape"]
        assert np.array_equal(torch.nonzero(hit).numpy(), ref[l + 1]["idx"].astype(np.int64).reshape(-1, 4)), (name, l)
        # the number of inputs an output gathers is what conv3d counted
        cnt = (ref[l + 1]["down"] >= 0).sum(1)
        assert np.array_equal(hit[hit > 0].numpy().astype(np.int64), cnt)


@pytest.mark.parametrize("name", [c["name"] for c in RC.CASES])
def test_case_fulfils_its_condition(name):
    c = RC.CASE[name]
    ref = RC.reference(name)
    cl = c["claims"]
    idx = c["idx"]
    if len(idx) > 1:
        k = RC.lin(idx, c["shape"])
        assert len(np.unique(k)) == len(k) and not np.all(k[1:] > k[:-1]), "level-0 rows are distinct and not sorted"
    assert idx.dtype == np.int32 and np.all(idx >= 0) and np.all(idx < np.array((c["batch"],) + c["shape"]))
    assert c["batch"] * float(np.prod(c["shape"])) < 4294967294.0
    if "cells0" in cl:
        assert set(cl["cells0"]) <= set(RC.lin(idx, c["shape"]).tolist())
    if "cells1" in cl:
        assert set(cl["cells1"]) <= set(RC.lin(ref[1]["idx"], ref[1]["shape"]).tolist())
    if cl.get("word_spans_rows"):
        assert any(RC.words_spanning(lv["idx"], lv["shape"], 2) > 0 for lv in ref[1:]), "no word holds cells of two y rows"
    if cl.get("word_spans_batches"):
        assert any(RC.words_spanning(lv["idx"], lv["shape"], 0) > 0 for lv in ref[1:]), "no word holds cells of two batches"
    if cl.get("full_neighbourhood"):
        assert any((lv["subm"] >= 0).all(1).any() for lv in ref), "no row with all 27 neighbours"
    if cl.get("full_words"):
        assert all(len(lv["idx"]) == c["batch"] * int(np.prod(lv["shape"])) for lv in ref)
    if cl.get("key_above_2_31"):
        assert RC.lin(idx, c["shape"]).max() >= 2 ** 31
    if "shapes" in cl:
        assert tuple(lv["shape"] for lv in ref) == cl["shapes"]
    if name == "empty":
        assert all(len(lv["idx"]) == 0 for lv in ref)
    if name in ("one", "three"):
        assert all(lv["shape"] == (1, 1, 1) and len(lv["idx"]) == c["batch"] for lv in ref)
    if name == "counters":
        sh = ref[1]["shape"]
        cells = int(np.prod(sh))
        words = (cells + 31) // 32
        assert sh == (4, 400, 700) and words == 35000 and (words + 255) // 256 == 137 == 2 * 64 + 9 and sh[2] % 32
    if name == "rounds":
        cells = 2 * int(np.prod(ref[1]["shape"]))
        blocks = ((cells + 31) // 32 + 1023) // 1024
        assert cells == 490000000 and blocks == 14954 and (blocks + 1023) // 1024 == 15
    if name == "high-key":
        assert 2 * int(np.prod(c["shape"])) == 2151680000 and c["levels"] == 2 and not c["chain"]
    # faces: a case that claims the grid corners has a voxel on every face of every batch, at every level
    if name == "corners":
        for lv in ref:
            for a in range(3):
                for b in range(c["batch"]):
                    col = lv["idx"][lv["idx"][:, 0] == b][:, 1 + a]
                    assert col.min() == 0 and col.max() == lv["shape"][a] - 1


@pytest.mark.parametrize("name,level", RC.TRUNCATED)
def test_truncated_cases_overflow(name, level):
    caps, ref = RC.truncated_caps(name, level)
    full = RC.reference(name)
    assert 0 < caps[level] < len(full[level]["idx"])
    for l, lv in enumerate(ref):
        assert (lv["total"] > caps[l]) == (l == level), "exactly the chosen level overflows"
        assert len(lv["idx"]) == min(lv["total"], caps[l])
    t = ref[level]
    assert np.array_equal(t["idx"], full[level]["idx"][:caps[level]]), "the first cap rows in ascending order"
    if level > 0:
        assert np.array_equal(t["down"], full[level]["down"][:caps[level]]), "their strided tables unchanged"
    cut = np.where(full[level]["subm"][:caps[level]] >= caps[level], -1, full[level]["subm"][:caps[level]])
    assert np.array_equal(t["subm"], cut) and (cut != full[level]["subm"][:caps[level]]).any()
    if level + 1 < len(ref):
        assert len(ref[level + 1]["idx"]) < len(full[level + 1]["idx"]), "the next level is built from the truncated set"


def test_hash_case_forms_a_chain_across_the_table_end():
    hc = RC.hash_wrap_case()
    idx, mask = hc["idx"], hc["mask"]
    assert mask == 1023 == RC.hash_slots(RC.HASH_CAP) - 1 and hc["homes"] == 279 and len(idx) == 60
    keys = RC.lin(idx, RC.HASH_SHAPE)
    assert len(np.unique(keys)) == 60
    home = RC.hash_u32(keys) & mask
    assert int((home >= RC.HASH_HOME).sum()) >= 40
    slots = RC.hash_insert_all(keys, mask)
    ent = np.stack([slots, np.zeros_like(slots)], 1)
    pos = {int(k): s for s, k in enumerate(slots.tolist()) if k != RC.EMPTY_KEY}
    for r, k in enumerate(keys.tolist()):
        ent[pos[k], 1] = r
    RC.check_hash_table(ent, keys, mask)
    # the chain from slot 1021 runs through 1023 into 0 .. 36 at least: 40 keys with 3 slots before the end
    run = 0
    while slots[run] != RC.EMPTY_KEY:
        run += 1
    assert run >= 37 and all(slots[s] != RC.EMPTY_KEY for s in (1021, 1022, 1023))
    # absent neighbours whose walk crosses the end of the table exist among the 27-neighbourhoods
    have = set(keys.tolist())
    d, h, w = RC.HASH_SHAPE
    crossing = 0
    for b, z, y, x in idx.tolist():
        for k in range(27):
            q = (b, z + k // 9 - 1, y + (k // 3) % 3 - 1, x + k % 3 - 1)
            if 0 <= q[1] < d and 0 <= q[2] < h and 0 <= q[3] < w:
                key = int(RC.lin(np.array([q]), RC.HASH_SHAPE)[0])
                if key not in have and (int(RC.hash_u32(key)) & mask) >= RC.HASH_HOME:
                    crossing += 1
    assert crossing > 0
    # a wrong table is noticed
    bad = ent.copy()
    bad[0, 0] = RC.EMPTY_KEY
    with pytest.raises(AssertionError):
        RC.check_hash_table(bad, keys, mask)


@pytest.mark.parametrize("n", RC.PAIRS_ROWS)
def test_pairs_cases(n):
    nbr, cap = RC.pairs_case(n)
    assert cap > n and nbr.shape == (cap, 27) and (nbr[n:] >= 0).any()
    pairs, num = RC.ref_pairs(nbr, n)
    assert num[RC.PAIRS_EMPTY_K] == 0 and num[RC.PAIRS_FULL_K] == n
    opairs, onum = orb.nbr_to_pairs(nbr[:n])
    assert np.array_equal(num, onum)
    for k in range(27):
        assert np.array_equal(pairs[k][0], opairs[k][0]) and np.array_equal(pairs[k][1], opairs[k][1])
        assert np.all(np.diff(pairs[k][1]) > 0)


def test_bf16_rounding_rules_agree():
    rng = np.random.default_rng(5)
    u = np.concatenate([RC.bf16_patterns(), rng.integers(0, 1 << 32, 200000, dtype=np.uint64).astype(np.uint32)])
    t = torch.from_numpy(u.view(np.int32).copy()).view(torch.float32).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    nan = RC.is_nan_bits32(u)
    assert nan.sum() >= 4 and np.array_equal(RC.is_nan_bits16(t), nan), "NaN stays NaN, nothing else becomes one"
    assert np.array_equal(t[~nan], RC.round_bf16_bits(u[~nan]))
    r = dict(zip(u.tolist(), RC.round_bf16_bits(u).tolist()))
    assert r[0x3F808000] == 0x3F80 and r[0x3F818000] == 0x3F82, "ties go to the even upper half"
    assert r[0x3F807FFF] == 0x3F80 and r[0x3F808001] == 0x3F81
    assert r[0x7F7FFFFF] == 0x7F80 and r[0xFF7FFFFF] == 0xFF80 and r[0x7F7F7FFF] == 0x7F7F
    assert r[0x00000000] == 0 and r[0x80000000] == 0x8000 and r[0x00008000] == 0 and r[0x00018000] == 2


@pytest.mark.parametrize("order", [0, 1])
def test_densify_reference_equals_the_oracle(order):
    for table in (RC.DENSIFY_F32, RC.DENSIFY_BF16):
        for shape, batch, chans, rows in table:
            for c in chans:
                for n in rows or RC.densify_rows(c):
                    cs = RC.densify_case(shape, batch, c, n, RC.SPECIAL_F32)
                    assert n * c <= 256 + 2 * c and len(np.unique(RC.lin(cs["idx"], shape))) == cs["cap"]
                    assert (cs["feats"][n:] != 0).all()
                    ref = RC.densify_ref_bits(cs["idx"], cs["feats"], n, shape, batch, order)
                    f = torch.from_numpy(cs["feats"][:n].view(np.int32).copy()).view(torch.float32)
                    o = onets.densify(f, cs["idx"][:n], shape, batch)
                    if order:
                        d, h, w = shape
                        o = o.view(batch, c, d, h, w).permute(0, 2, 1, 3, 4).reshape(batch, c * d, h, w)
                    assert np.array_equal(o.contiguous().view(torch.int32).numpy().view(np.uint32), ref)
    rows = {c: RC.densify_rows(c) for c in (1, 16, 64)}
    assert all(any(n * c < 256 for n in r if n) and any(n * c > 256 for n in r) for c, r in rows.items())
    assert (2 * 3 * 3 * 5 * 7 * 4) % 16 != 0 and (3 * 16 * 5 * 8 * 16 * 4) % 16 == 0 and (4 * 6) % 8 == 0 and (5 * 7) % 8 != 0


@pytest.mark.parametrize("t", RC.VOXEL_MEAN_T)
def test_voxel_mean_twin_equals_the_oracle(t):
    for ndim, nfeat in RC.VOXEL_MEAN_DIMS:
        for m in RC.VOXEL_MEAN_M:
            v, num = RC.voxel_mean_case(m, t, ndim)
            assert num.min() >= 1 and num.max() <= t and (m < t or set(num.tolist()) == set(range(1, t + 1)))
            assert all((v[i, num[i]:] == 0).all() and (v[i, :num[i]] != 0).all() for i in range(m))
            twin = RC.voxel_mean_twin(v, num, nfeat)
            assert np.array_equal(clib.voxel_mean(v, num, nfeat).view(np.int32), twin.view(np.int32)), (t, ndim, nfeat, m)
