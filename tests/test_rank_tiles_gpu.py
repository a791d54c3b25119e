"""The cosine GEMM's two-launch tile split (launch_tiles, csrc/rank_common.h) under every epilogue and loop family, on the GPU.

A call is cut in two when it has more tiles than the device has resident workgroup slots; production shapes aside, no search of
the suite is that large.  mi355_rank_set_round_slots moves the cut (and nothing else), so that small shapes run a main launch of
128-query tiles and a tail launch of 64-query tiles; mi355_rank_last_tiles reports the cut that was taken.  On lattice rows
(tests/rank_tiles_ref.py) every score is an exact multiple of 1 / 16, so each result must equal the numpy reference element for
element and bit for bit, and the same call without the override (one launch).  Before every call under test its outputs, its
candidate buffer and its whole workspace hold 0xFF bytes: a tile that is never written reads as NaN / -1 instead of as the
previous call's correct values.  No tolerance appears in this file."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import imageretrievalresearch_amd as M
import rank_tiles_ref as ref
from imageretrievalresearch_amd import lib
from imageretrievalresearch_amd._lib import RankFilter, stream_ptr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 1e-6
GEMV, SPLIT, EXACT, PREP, F16_GEMM, FUSED, BITONIC = 1, 2, 3, 4, 5, 0x100, 0x200

# loop family -> (kind, D, raw rows (+-1, gallery_is_normalized = 0) or unit rows (+-0.25), MI355_RANK_EXACT_F32)
FAMILIES = {
    "split48": ("f32", 48, False, False), "split100raw": ("f32", 100, True, False),
    "exactvec48raw": ("f32", 48, True, True), "exact70": ("f32", 70, False, False),        # dim % 4: the non-VEC fp32 loop
    "f16-48": ("f16", 48, False, False), "f16-70": ("f16", 70, False, False), "f16-100": ("f16", 100, False, False),
    "prepared48": ("prepared", 48, False, False),
}
PATHS = {"split48": SPLIT, "split100raw": SPLIT, "exactvec48raw": EXACT, "exact70": EXACT, "f16-48": F16_GEMM, "f16-70": F16_GEMM,
         "f16-100": F16_GEMM, "prepared48": PREP}


def _epilogues(fam):
    kind = FAMILIES[fam][0]
    if kind == "prepared":                                  # the planes serve the unfiltered fused selection only
        return ["topk1", "topk2", "topk3", "topk8"]
    if kind == "f16":                                       # fp16 rows have no slab entry: their slab is the k = 9 search
        return [e for e in ref.EPILOGUES if e != "slab"]
    return ref.EPILOGUES


MATRIX = [(fam, c, e) for fam in FAMILIES for c in ref.CASES for e in _epilogues(fam)]
BLOCKS = [(fam, c, e) for fam in ("split48", "exact70", "f16-70") for c in ref.BLOCK_CASES for e in ("ranks", "nearest")]

# The DMA ring of the split and the prepared loop (dma_ring, csrc/rank_common.h) at every number of 16-wide k-steps the D = 48
# of the matrix (3 steps) leaves out: D = 16, 20, 32, 64, 80 are 1, 2 (zeros past D inside the second), 2, 4 and 5 steps.  At 2 and
# 4 steps the A ring of 3 of the 64-query kernels takes its extra prologue piece and then issues nothing in the loop, at 4 and 5
# the B ring of 3 wraps.  Outside MATRIX: two cases and a few epilogues each, under the forced cut (both tile heights run).
STEP_D = (16, 20, 32, 64, 80)
STEP_EPILOGUES = {"split": ("f32", SPLIT, ["slab", "topk3", "filt2", "range"]), "prepared": ("prepared", PREP, ["topk3", "topk8"])}
STEPS = []
for _D in STEP_D:
    for _name, (_kind, _path, _epis) in STEP_EPILOGUES.items():
        FAMILIES["%s%d" % (_name, _D)], PATHS["%s%d" % (_name, _D)] = (_kind, _D, False, False), _path
        STEPS += [("%s%d" % (_name, _D), c, e) for c in (ref.CASES[0], ref.CASES[2]) for e in _epis]


@pytest.fixture(autouse=True)
def _restore_the_override():
    yield
    assert lib().mi355_rank_set_round_slots(0) == 0


def _poison(shape, dtype):
    t = torch.empty(shape, dtype=dtype, device=DEV)
    t.view(-1).view(torch.uint8).fill_(0xFF)
    return t


def _np(t):
    return t.cpu().numpy()


def _ok(status):
    assert status == 0, lib().mi355_last_error()


def _tiles():
    out = (C.c_int * 5)()
    assert lib().mi355_rank_last_tiles(out, 5) == 5
    return tuple(out)


class Inputs:
    """One data set on the device, as one loop family reads it."""

    def __init__(self, d, fam):
        self.d, self.fam = d, fam
        self.kind, D, self.raw, self.exact = FAMILIES[fam]
        assert D == d.D
        self.q = torch.from_numpy(d.rows("q", self.raw)).to(DEV)
        g = torch.from_numpy(d.rows("g", self.raw)).to(DEV)
        self.keep = g
        if self.kind == "f16":
            self.keep = M.Gallery(D, DEV, dtype=torch.float16).add(g)
            self.g = self.keep._buf.data_ptr()
        elif self.kind == "prepared":
            self.keep = M.PreparedGallery(g)
            self.g = self.keep.planes.data_ptr()
        else:
            self.g = g.data_ptr()
        self.norm = () if self.kind == "f16" else (0 if self.raw else 1,)
        self.ql, self.gl = torch.from_numpy(d.ql).to(DEV), torch.from_numpy(d.gl).to(DEV)
        self.excl = torch.from_numpy(d.excl).to(DEV)
        self.thr = torch.from_numpy(d.thr).to(DEV)
        self.sfx = "_f16" if self.kind == "f16" else ""

    def filt(self, mode):
        f = RankFilter()
        f.label_mode = mode
        if mode != ref.ANY:
            f.query_labels, f.gallery_labels = self.ql.data_ptr(), self.gl.data_ptr()
        f.exclude = self.excl.data_ptr()
        return f

    def ws(self, name, *args):
        n = int(getattr(lib(), name)(*args))
        assert n > 0
        return _poison((n + 4096,), torch.uint8), n + 4096

    # Each method runs one epilogue from poisoned buffers and returns (the result as a tuple of numpy arrays, the rank path, the
    # cut of every GEMM-bearing call).
    def slab(self):
        d, L = self.d, lib()
        out = _poison((d.Q, d.G), torch.float32)
        w, n = self.ws("mi355_rank_workspace_bytes", d.Q, d.G, d.D, 0)
        _ok(L.mi355_cosine_scores(self.q.data_ptr(), d.Q, self.g, d.G, d.D, *self.norm, EPS, out.data_ptr(), w.data_ptr(), n,
                                  stream_ptr(DEV)))
        return (_np(out),), L.mi355_rank_last_path(), [_tiles()]

    def topk(self, k, filtered):
        d, L = self.d, lib()
        ov, oi = _poison((d.Q, k), torch.float32), _poison((d.Q, k), torch.int64)
        w, n = self.ws("mi355_rank_f16_workspace_bytes" if self.kind == "f16" else "mi355_rank_workspace_bytes", d.Q, d.G, d.D, k)
        tailargs = (ov.data_ptr(), oi.data_ptr(), w.data_ptr(), n, stream_ptr(DEV))
        f = self.filt(d.mode)
        if self.kind == "prepared":
            assert not filtered
            _ok(L.mi355_rank_topk_prepared(self.q.data_ptr(), d.Q, self.g, d.G, d.D, k, EPS, d.off, *tailargs))
        elif filtered:
            _ok(getattr(L, "mi355_rank_topk%s_filtered" % self.sfx)(self.q.data_ptr(), d.Q, self.g, d.G, d.D, *self.norm, k, EPS, d.off,
                                                                  C.byref(f), *tailargs))
        else:
            _ok(getattr(L, "mi355_rank_topk" + self.sfx)(self.q.data_ptr(), d.Q, self.g, d.G, d.D, *self.norm, k, EPS, d.off, *tailargs))
        return (_np(ov), _np(oi)), L.mi355_rank_last_path(), [_tiles()]

    def roc(self):
        d, L = self.d, lib()
        T = d.thr.shape[0]
        hist = _poison((2, T + 1), torch.int64)
        w, n = self.ws("mi355_roc_pairs%s_workspace_bytes" % self.sfx, d.Q, d.G, d.D)
        _ok(getattr(L, "mi355_roc_pairs_hist" + self.sfx)(self.q.data_ptr(), d.Q, self.g, d.G, d.D, *self.norm, EPS, self.ql.data_ptr(),
                                                         self.gl.data_ptr(), self.excl.data_ptr(), d.off,
                                                         d.thr.ctypes.data_as(C.POINTER(C.c_double)), self.thr.data_ptr(), T,
                                                         hist.data_ptr(), w.data_ptr(), n, stream_ptr(DEV)))
        return (_np(hist),), L.mi355_rank_last_path(), [_tiles()]

    def _range(self, entry, thr, f, cap):
        """One range pass and its compaction: (offsets, indices, scores), the cut."""
        d, L = self.d, lib()
        cand = _poison((2 * cap,), torch.int64)
        w, n = self.ws("mi355_range%s_workspace_bytes" % self.sfx, d.Q, d.G, d.D)
        nnz = C.c_int64(-1)
        _ok(getattr(L, entry + self.sfx)(self.q.data_ptr(), d.Q, self.g, d.G, d.D, *self.norm, EPS, *thr, d.off, C.byref(f), cand.data_ptr(),
                                         cap, C.byref(nnz), w.data_ptr(), n, stream_ptr(DEV)))
        tiles, path = _tiles(), L.mi355_rank_last_path()
        assert 0 <= nnz.value <= cap, (nnz.value, cap)            # (cap is the reference's count: more hits are wrong hits)
        offsets = _poison((d.Q + 1,), torch.int64)
        indices, scores = _poison((max(nnz.value, 1),), torch.int64), _poison((max(nnz.value, 1),), torch.float32)
        _ok(L.mi355_range_compact(cand.data_ptr(), cap, d.Q, nnz.value, d.off, w.data_ptr(), n, offsets.data_ptr(), indices.data_ptr(),
                                  scores.data_ptr(), stream_ptr(DEV)))
        assert int(offsets[-1]) == nnz.value
        return (_np(offsets), _np(indices)[: nnz.value], _np(scores)[: nnz.value]), path, tiles

    def range(self):
        d, out, tiles = self.d, (), []
        want = ref.reference(d, "range")
        for t, cap in ((d.t_on, want[1].shape[0]), (d.t_between, want[4].shape[0])):
            r, path, tl = self._range("mi355_cosine_range", (float(t),), self.filt(d.mode), cap + 8)
            out, tiles = out + r, tiles + [tl]
        return out, path, tiles

    def ranks(self, qblock=0):
        d, L = self.d, lib()
        want = ref.reference(d, "ranks")
        (offsets, indices, scores), path, tl0 = self._range("mi355_positives_range", (), self.filt(ref.SAME), want[1].shape[0] + 8)
        nnz = indices.shape[0]
        it, st = torch.from_numpy(indices).to(DEV), torch.from_numpy(scores).to(DEV)
        keys = _poison((max(nnz, 1),), torch.int64)
        _ok(L.mi355_rank_positives_keys(it.data_ptr(), st.data_ptr(), nnz, d.off, keys.data_ptr(), stream_ptr(DEV)))
        row_keys = _np(keys)[:nnz].view(np.uint64)
        sorted_keys = row_keys.copy()
        for q in range(d.Q):                                       # each query's composites in rank order: descending
            sorted_keys[offsets[q]:offsets[q + 1]] = np.sort(row_keys[offsets[q]:offsets[q + 1]])[::-1]
        kt, ot = torch.from_numpy(sorted_keys.view(np.int64)).to(DEV), torch.from_numpy(offsets).to(DEV)
        before = _poison((max(nnz, 1),), torch.int32)
        w, n = self.ws("mi355_rank_positives%s_workspace_bytes" % self.sfx, d.Q, d.G, d.D)
        _ok(getattr(L, "mi355_rank_positives" + self.sfx)(self.q.data_ptr(), d.Q, self.g, d.G, d.D, *self.norm, EPS, self.ql.data_ptr(),
                                                         self.gl.data_ptr(), self.excl.data_ptr(), d.off, ot.data_ptr(),
                                                         offsets.ctypes.data_as(C.POINTER(C.c_int64)), kt.data_ptr(), nnz,
                                                         before.data_ptr(), qblock, w.data_ptr(), n, stream_ptr(DEV)))
        tl1, path1 = _tiles(), L.mi355_rank_last_path()
        assert path1 == path
        ranks, ap, first = _poison((max(nnz, 1),), torch.int64), _poison((d.Q,), torch.float64), _poison((d.Q,), torch.int64)
        _ok(L.mi355_rank_positives_finalize(ot.data_ptr(), before.data_ptr(), d.Q, nnz, ranks.data_ptr(), ap.data_ptr(), first.data_ptr(),
                                            stream_ptr(DEV)))
        return ((offsets, indices, scores, row_keys, _np(before)[:nnz].view(np.uint32), _np(ranks)[:nnz], _np(ap), _np(first)), path,
                [tl0, tl1])

    def nearest(self, qblock=0):
        d, L = self.d, lib()
        assign, score = _poison((d.G,), torch.int64), _poison((d.G,), torch.float32)
        w, n = self.ws("mi355_nearest_centroid%s_workspace_bytes" % self.sfx, d.Q, d.G, d.D)
        _ok(getattr(L, "mi355_nearest_centroid" + self.sfx)(self.q.data_ptr(), d.Q, self.g, d.G, d.D, *self.norm, EPS, qblock,
                                                           assign.data_ptr(), score.data_ptr(), w.data_ptr(), n, stream_ptr(DEV)))
        return (_np(assign), _np(score)), L.mi355_rank_last_path(), [_tiles()]

    def run(self, epi, slots, qblock=0):
        """Epilogue epi with the cut forced to slots (0: the device's own)."""
        assert lib().mi355_rank_set_round_slots(slots) == 0
        try:
            if epi == "slab":
                return self.slab()
            if epi[:4] in ("topk", "filt"):
                return self.topk(int(epi[4:]), epi[:4] == "filt")
            if epi in ("ranks", "nearest"):
                return getattr(self, epi)(qblock)
            return getattr(self, epi)()
        finally:
            assert lib().mi355_rank_set_round_slots(0) == 0

    def path(self, epi):
        p = PATHS[self.fam]
        if epi[:4] in ("topk", "filt"):
            p |= FUSED if int(epi[4:]) <= 8 else BITONIC
        return p


@functools.lru_cache(maxsize=4)
def _inputs(fam, case, qblock=0):
    return Inputs(ref.case_data(*case, FAMILIES[fam][1], qblock), fam)


def _env(monkeypatch, fam):
    if FAMILIES[fam][3]:
        monkeypatch.setenv("MI355_RANK_EXACT_F32", "1")
    else:
        monkeypatch.delenv("MI355_RANK_EXACT_F32", raising=False)


def _expected_tiles(epi, slots, Q, G, qblock):
    """The cut of every GEMM-bearing call of an epilogue: the range and positives passes take all Q queries in one call, the
    counting pass and the nearest centroid go query_block at a time and report their last block."""
    last = ref.blocks(Q, qblock)[-1][1]
    whole, blocked = (slots,) + ref.report(Q, G, slots), (slots,) + ref.report(last, G, slots)
    return {"range": [whole, whole], "ranks": [whole, blocked], "nearest": [blocked]}.get(epi, [whole])


def _check_forced(monkeypatch, fam, case, epi, qblock=0):
    slots, Q, G = case
    _env(monkeypatch, fam)
    x = _inputs(fam, case, qblock)
    want = ref.reference(x.d, epi)
    got, path, tiles = x.run(epi, slots, qblock)
    assert path == x.path(epi), hex(path)
    assert tiles == _expected_tiles(epi, slots, Q, G, qblock), tiles
    if not qblock or epi != "nearest":
        assert any(t[3] > 0 for t in tiles)                       # a tail launch ran
    assert ref.same_result(got, want)
    one, path1, tiles1 = x.run(epi, 0, qblock)                    # the device's own slots: one launch at these shapes
    assert path1 == path and all(t[3] == 0 and t[0] >= 256 for t in tiles1), tiles1
    assert ref.same_result(one, got)


def test_the_lattice_premise():
    """l2_normalize_rows of the +-1 rows is the +-0.25 rows bit for bit (norm 4, 1 / 4 and x / 4 exact), and the fp16 gallery of
    either is the same fp16 rows: the raw and the unit variant of a case are the same rows to every kernel."""
    for D in (48, 70, 100) + STEP_D:
        d = ref.case_data(*ref.CASES[0], D)
        for which in "qg":
            raw, unit = d.rows(which, True), d.rows(which, False)
            got = M.l2_normalize_rows(torch.from_numpy(raw).to(DEV))
            assert ref.same_result((_np(got),), (unit,))
            again = M.l2_normalize_rows(torch.from_numpy(unit).to(DEV))
            assert ref.same_result((_np(again),), (unit,))
        a = M.Gallery(D, DEV, dtype=torch.float16).add(torch.from_numpy(d.rows("g", True)).to(DEV))
        b = M.Gallery(D, DEV, dtype=torch.float16).add(torch.from_numpy(d.rows("g", False)).to(DEV))
        assert torch.equal(a._buf.view(torch.int16), b._buf.view(torch.int16))
        assert np.array_equal(_np(a.data.float()), d.rows("g", False))


@pytest.mark.parametrize("fam,case,epi", MATRIX, ids=lambda v: v if isinstance(v, str) else "s%d-q%d-g%d" % v)
def test_forced_split(fam, case, epi, monkeypatch):
    _check_forced(monkeypatch, fam, case, epi)


@pytest.mark.parametrize("fam,case,epi", STEPS, ids=lambda v: v if isinstance(v, str) else "s%d-q%d-g%d" % v)
def test_forced_split_at_every_k_step_count(fam, case, epi, monkeypatch):
    _check_forced(monkeypatch, fam, case, epi)


@pytest.mark.parametrize("fam,case,epi", BLOCKS,ids=lambda v: v if isinstance(v, str) else "s%d-q%d-g%d-b%d" % v)
def test_forced_split_over_several_query_blocks(fam, case, epi, monkeypatch):
    _check_forced(monkeypatch, fam, case[:3], epi, case[3])


# ---------------------------------------------------------------- Gaussian rows: a score depends on its two rows only
class GaussData:
    def __init__(self, Q, G, D, seed):
        rng = np.random.default_rng(seed)
        self.Q, self.G, self.D, self.off, self.mode = Q, G, D, 17, ref.ANY
        self.q = rng.standard_normal((Q, D)).astype(np.float32)
        self.g = rng.standard_normal((G, D)).astype(np.float32)
        self.unit = (self.g / np.sqrt((self.g.astype(np.float64) ** 2).sum(1))[:, None]).astype(np.float32)
        self.ql, self.gl = np.zeros(Q, np.int64), np.zeros(G, np.int64)
        self.excl = np.full(Q, -1, np.int64)
        self.thr = np.array([0.0])
        self.t_on = self.t_between = 0.2
        self.cache = {}

    def rows(self, which, raw):
        return self.q if which == "q" else self.g if raw else self.unit


@pytest.mark.parametrize("case", [ref.CASES[1], ref.CASES[2], ref.CASES[5]], ids=lambda c: "s%d-q%d-g%d" % c)
@pytest.mark.parametrize("fam", ["split48", "exactvec48raw", "exact70", "f16-70", "prepared48"])
def test_gaussian_rows_keep_their_bits_across_the_cut(fam, case, monkeypatch):
    """The header's promise - a score depends on its query row and its gallery row only - on rows whose scores do round: the
    slab, the top-k values and indices and the range scores are the same bits with one launch and with two."""
    slots, Q, G = case
    _env(monkeypatch, fam)
    d = GaussData(Q, G, FAMILIES[fam][1], 5 + slots)
    x = Inputs(d, fam)
    epis = ["topk3", "topk8"] if fam == "prepared48" else [e for e in ("slab", "topk1", "topk3", "topk9") if e in _epilogues(fam)]
    for epi in epis:
        two, path, tiles = x.run(epi, slots)
        one, path1, tiles1 = x.run(epi, 0)
        assert path == path1 == x.path(epi) and tiles[0][3] > 0 and tiles1[0][3] == 0
        assert ref.same_result(two, one), epi
    if fam != "prepared48":
        # (the capacity comes from the single launch here: there is no exact reference for rows that round)
        one, _, tiles1 = x._range("mi355_cosine_range", (0.2,), x.filt(ref.ANY), Q * G)
        assert lib().mi355_rank_set_round_slots(slots) == 0
        two, _, tiles = x._range("mi355_cosine_range", (0.2,), x.filt(ref.ANY), one[1].shape[0] + 8)
        assert tiles[3] > 0 and tiles1[3] == 0 and one[1].shape[0] > 0
        assert ref.same_result(two, one)


# ---------------------------------------------------------------- the device's own split
OWN_Q, OWN_D = 1400, 48


@functools.lru_cache(maxsize=2)
def _own_data(G):
    return ref.Data(OWN_Q, G, OWN_D, 4242, None, ref.SAME)


@functools.lru_cache(maxsize=2)
def _own_inputs(fam, G):
    return Inputs(_own_data(G), fam)


@pytest.mark.parametrize("epi,fam", [(e, fam) for e in ref.EPILOGUES for fam in ("split48", "f16-48") if e in _epilogues(fam)])
def test_the_devices_own_split(epi, fam, monkeypatch):
    """No override: 11 query tiles of 128 and just enough column tiles that the device's own slot count leaves a tail.  The slots
    are those of the epilogue's own kernel, read from a small probe call; the positives pass in front of the ranks is the range
    kernel, whose own case is "range"."""
    _env(monkeypatch, fam)
    _, _, probe = _inputs(fam, ref.CASES[0]).run(epi, 0)
    assert all(t[0] >= 256 and t[3] == 0 for t in probe), probe
    slots = probe[-1][0]
    G = (slots // 11 + 3) * 128 - 5
    assert G <= 16000
    x = _own_inputs(fam, G)
    got, path, tiles = x.run(epi, 0)
    assert path == x.path(epi)
    assert tiles == [(p[0],) + ref.report(OWN_Q, G, p[0]) for p in probe], tiles
    assert tiles[-1][3] > 0 and tiles[-1][1] == 11 and tiles[-1][4] == 22, tiles
    assert ref.same_result(got, ref.reference(x.d, epi))
