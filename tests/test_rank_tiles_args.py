"""The cosine GEMM's two-launch tile split, the parts that need no GPU: the developer entries mi355_rank_round_split,
mi355_rank_set_round_slots and mi355_rank_last_tiles and their argument checks, the properties of whole_round_tiles, that the
restated rank_tile_of covers every launch of the GPU matrix exactly once, that the matrix reaches every split class, and that
the references of tests/rank_tiles_ref.py tell each modelled seam bug from the sound result."""
import ctypes
import threading

import numpy as np
import pytest

import rank_tiles_ref as ref
from helpers import header_symbols
from imageretrievalresearch_amd import _lib

NEW = ["mi355_rank_round_split", "mi355_rank_set_round_slots", "mi355_rank_last_tiles"]
ALL_CASES = [c + (0,) for c in ref.CASES] + ref.BLOCK_CASES


def test_symbols_declared_bound_and_exported():
    for name in NEW:
        assert name in header_symbols()
        assert name in _lib.PROTOTYPES
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    assert _lib.lib().mi355_abi_version() == 3


def test_set_round_slots_arguments():
    L = _lib.lib()
    try:
        assert L.mi355_rank_set_round_slots(-1) != 0
        assert b"slots" in L.mi355_last_error()
        assert L.mi355_rank_set_round_slots(-(1 << 31)) != 0
        assert L.mi355_rank_set_round_slots(7) == 0
        assert L.mi355_rank_set_round_slots((1 << 31) - 1) == 0
    finally:
        assert L.mi355_rank_set_round_slots(0) == 0


def test_last_tiles_arguments():
    L = _lib.lib()
    out = (ctypes.c_int * 8)(*([-7] * 8))
    assert L.mi355_rank_last_tiles(None, 5) < 0
    assert L.mi355_rank_last_tiles(out, 0) < 0
    assert L.mi355_rank_last_tiles(out, -3) < 0
    assert list(out) == [-7] * 8                                  # a rejected call writes nothing
    assert L.mi355_rank_last_tiles(out, 2) == 2 and list(out)[2:] == [-7] * 6
    assert L.mi355_rank_last_tiles(out, 8) == 5 and list(out)[5:] == [-7] * 3
    fresh = []                                                    # the record is per thread: a new thread has made no call

    def read():
        o = (ctypes.c_int * 5)(*([-7] * 5))
        fresh.append((L.mi355_rank_last_tiles(o, 5), list(o)))

    t = threading.Thread(target=read)
    t.start()
    t.join()
    assert fresh == [(5, [0] * 5)]


def test_round_split_arguments():
    L = _lib.lib()
    for bad in ((-1, 1, 1), (4, 0, 1), (4, -1, 1), (4, 1, 0), (4, 1, -2)):
        assert L.mi355_rank_round_split(*bad) == -1
    assert L.mi355_rank_round_split(0, 1, 1) == 0
    assert L.mi355_rank_round_split(9, 1, 6) == 6 and L.mi355_rank_round_split(13, 2, 8) == 12
    assert L.mi355_rank_round_split(23, 3, 20) == 20


def test_round_split_properties():
    L = _lib.lib()
    ntxs = list(range(0, 70)) + [255, 256, 257, 782, 1564, 23438, (1 << 24) - 1]
    nys = list(range(1, 13)) + [128, 256]
    slotss = list(range(1, 41)) + [255, 256, 512, 768, 1024, 1 << 20]
    n = 0
    for ntx in ntxs:
        for ny in nys:
            for slots in slotss:
                x1 = L.mi355_rank_round_split(ntx, ny, slots)
                tiles = ntx * ny
                assert x1 == ref.round_split(ntx, ny, slots)
                assert 0 <= x1 <= ntx
                fits = tiles <= slots or tiles % slots == 0
                assert (x1 == ntx) == fits, (ntx, ny, slots, x1)
                if not fits:
                    whole = tiles // slots * slots
                    assert x1 * ny <= whole < (x1 + 1) * ny, (ntx, ny, slots, x1)
                n += 1
    assert n == len(ntxs) * len(nys) * len(slotss)


def test_the_matrix_reaches_every_split_class():
    assert ref.classes(ref.CASES) == ref.CLASSES
    for slots, Q, G, qb in ref.BLOCK_CASES:
        calls = ref.blocks(Q, qb)
        assert len(calls) >= 2 and ref.report(calls[0][1], G, slots)[2] > 0          # several blocks, and they split


@pytest.mark.parametrize("slots,Q,G,qb", ALL_CASES)
def test_tile_of_is_a_bijection_on_every_launch(slots, Q, G, qb):
    for q0, qn in ref.blocks(Q, qb):
        ls = ref.launches(qn, G, slots)
        assert sum(xt for _, _, xt, _ in ls) == ref.cdiv(G, ref.BN)
        for MT, x0, xt, ny in ls:
            got = sorted(ref.tile_of(L, xt, ny) for L in range(xt * ny))
            assert got == [(tx, ty) for tx in range(xt) for ty in range(ny)]
            assert ny == ref.cdiv(qn, 64 * MT)
        # every (query, gallery row) pair lies in exactly one workgroup's tile
        times = np.zeros((qn, G), np.int32)
        for m0, m1, n0, n1, col in ref.workgroups(qn, G, slots):
            times[m0:m1, n0:n1] += 1
            assert col == n0 // ref.BN
        assert (times == 1).all()


def test_tile_of_is_a_bijection_in_general():
    for nt in list(range(1, 30)) + [64, 65, 71]:
        for ny in (1, 2, 3, 5, 11):
            got = sorted(ref.tile_of(L, nt, ny) for L in range(nt * ny))
            assert got == [(tx, ty) for tx in range(nt) for ty in range(ny)]
            # the query tiles of one column tile of a full group lie 8 apart: they start in the same round, on one XCD
            if nt >= 8:
                assert [ref.tile_of(L, nt, ny) for L in range(0, 8 * ny, 8)] == [(0, ty) for ty in range(ny)]


@pytest.mark.parametrize("epi", ref.EPILOGUES)
@pytest.mark.parametrize("slots,Q,G,qb", ALL_CASES)
def test_the_references_tell_each_modelled_bug(slots, Q, G, qb, epi):
    """The tile-by-tile model of the epilogue equals the reference for any cut, and each modelled bug - tail tiles placed from
    column 0, the tail launched with the main launch's ny, tables indexed without x0, a tie at the seam resolved to the higher
    index, a tail tile counted twice - changes the result of every case it can reach."""
    d = ref.case_data(slots, Q, G, 48, qb)
    want = ref.reference(d, epi)
    assert ref.same_result(ref.run_model(d, epi, slots, None, qb), want)
    assert ref.same_result(ref.run_model(d, epi, 0, None, qb), want)             # one launch
    reached = 0
    for bug in ref.BUGS:
        if ref.applies(bug, epi):
            assert not ref.same_result(ref.run_model(d, epi, slots, bug, qb), want), bug
            reached += 1
    assert reached >= 2


def test_every_bug_reaches_some_epilogue_and_the_inputs_are_lattice_rows():
    for bug in ref.BUGS:
        assert any(ref.applies(bug, e) for e in ref.EPILOGUES)
    d = ref.case_data(*ref.CASES[2], 100)
    for x in (d.qi, d.gi):
        assert ((x != 0).sum(1) == ref.NNZ).all() and set(np.unique(x)) == {-1, 0, 1}
    for raw in (False, True):
        q, g = d.rows("q", raw).astype(np.float64), d.rows("g", raw).astype(np.float64)
        assert (np.sqrt((g * g).sum(1)) == (4.0 if raw else 1.0)).all()
        s = (q @ g.T) / (16.0 if raw else 1.0)
        assert np.array_equal(s * 16, d.S)                                        # every score is S / 16, exactly
    assert np.array_equal(ref.f32(d.S).astype(np.float64) * 16, d.S)
    assert (np.diff(d.thr) == 0).any() and (d.thr * 16 == np.rint(d.thr * 16)).any() and (d.thr * 16 != np.rint(d.thr * 16)).any()
    # ties across the seam, and pads: what the planted rows are for
    v, i = ref.topk_ref(d, 2)
    assert (v[:4] == 1.0).all() and ((i[:4, 0] - d.off) < ref.seam(d.Q, d.G, ref.CASES[2][0])).all()
    assert ((i[:4, 1] - d.off) >= ref.seam(d.Q, d.G, ref.CASES[2][0])).all()
    fv, fi = ref.topk_ref(d, 3, d.eligible(ref.SAME))
    assert (fi[d.Q - 1] == -1).all() and np.isneginf(fv[d.Q - 1]).all() and (fi[d.Q - 2] == -1).sum() == 1
