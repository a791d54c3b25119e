"""Ragged uint8 batches (mi355_resize_batch_u8, mi355_model_forward_images): ABI surface and argument checks, no GPU needed."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from helpers import ROOT
from imageretrievalresearch_amd import _lib

NEW = ["mi355_resize_batch_workspace_bytes", "mi355_resize_batch_u8", "mi355_model_forward_images_workspace_bytes",
       "mi355_model_forward_images"]
FAKE = 0x10000        # a non-null "device" address: every call below must fail its checks before touching it


def _desc(sizes, offset=0):
    out, off = [], offset
    for h, w in sizes:
        out.append((off, h, w))
        off += h * w * 3
    return np.ascontiguousarray(np.array(out, dtype=np.int64)), off


def _p(a):
    return a.ctypes.data


def test_new_symbols_in_header_binding_and_library():
    hdr = open(f"{ROOT}/include/mi355_retrieval.h").read()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if " T " in ln}
    for name in NEW:
        assert f"{name}(" in hdr and name in _lib.PROTOTYPES and name in exported, name


def _resize(L, desc, nbytes, B=None, oh=224, ow=224, pad=0, fill=255, px=FAKE, dd=FAKE, out=FAKE, ws=FAKE, wsb=1 << 40):
    dh = _p(desc) if desc is not None else None
    B = (len(desc) if desc is not None else 1) if B is None else B
    return L.mi355_resize_batch_u8(px, nbytes, dh, dd, B, oh, ow, pad, fill, out, ws, wsb, None)


@pytest.mark.parametrize("case,msg", [
    (dict(px=None), b"null"), (dict(dd=None), b"null"), (dict(desc=None), b"null"), (dict(out=None), b"null"),
    (dict(B=0), b"B=0"), (dict(oh=0), b"output size"), (dict(ow=16385), b"output size"), (dict(fill=256), b"fill"),
    (dict(fill=-1), b"fill"), (dict(ws=None), b"workspace"), (dict(wsb=16), b"workspace"),
])
def test_resize_batch_rejects_bad_arguments(case, msg):
    L = _lib.lib()
    desc, nbytes = _desc([(224, 150), (97, 224)])
    kw = dict(desc=desc)
    kw.update(case)
    assert _resize(L, kw.pop("desc"), nbytes, **kw) != 0
    assert msg in L.mi355_last_error(), L.mi355_last_error()


@pytest.mark.parametrize("sizes,shift,nbytes_delta,msg", [
    ([(0, 224)], 0, 0, b"bad size"), ([(224, 0)], 0, 0, b"bad size"), ([(16385, 2)], 0, 0, b"bad size"),
    ([(5, 7), (3, 3)], 0, -1, b"outside"), ([(5, 7)], -3, 0, b"outside"), ([(5, 7)], 1, 0, b"outside"),
])
def test_descriptors_are_checked(sizes, shift, nbytes_delta, msg):
    L = _lib.lib()
    desc, nbytes = _desc(sizes)
    desc[:, 0] += shift
    assert _resize(L, desc, nbytes + nbytes_delta) != 0
    assert msg in L.mi355_last_error(), L.mi355_last_error()


def test_forward_images_rejects_bad_arguments():
    L = _lib.lib()
    m, sw = C.c_void_p(), C.c_void_p()
    assert L.mi355_model_create(b"efficientnet_b3a", 0, C.byref(m)) == 0
    assert L.mi355_model_create(b"swin_base_patch4_window7_224", 0, C.byref(sw)) == 0
    mean, std = (C.c_float * 3)(0.5, 0.5, 0.5), (C.c_float * 3)(0.2, 0.2, 0.2)
    zstd = (C.c_float * 3)(0.2, 0.0, 0.2)
    desc, nbytes = _desc([(224, 224), (224, 150), (97, 224)])
    mixed, mixed_bytes = _desc([(224, 224), (200, 150)])
    small, small_bytes = _desc([(200, 150)])

    def call(model=m, transform=0, size=224, fill=255, st=std, cw=None, ws=FAKE, wsb=1 << 40, d=desc, nb=nbytes, B=None,
             px=FAKE, dd=FAKE, out=FAKE):
        return L.mi355_model_forward_images(model, px, nb, _p(d), dd, len(d) if B is None else B, transform, size, fill, mean,
                                            st, cw, 0, out, None, ws, wsb, None)
    try:
        for kw, msg in [(dict(model=None), b"null"), (dict(out=None), b"null"), (dict(px=None), b"null"),
                        (dict(dd=None), b"null"), (dict(B=0), b"B=0"), (dict(transform=3), b"transform"),
                        (dict(transform=-1), b"transform"), (dict(fill=300), b"fill"), (dict(fill=-1), b"fill"),
                        (dict(st=zstd), b"std"), (dict(nb=nbytes - 1), b"outside"),
                        (dict(d=mixed, nb=mixed_bytes), b"one S per batch"),
                        (dict(model=sw, cw=FAKE), b"conv_input"),
                        (dict(model=sw, d=small, nb=small_bytes), b"224"),
                        (dict(model=sw, transform=1, size=112), b"224"),
                        (dict(transform=1, size=0), b"out_size"), (dict(transform=2, size=16385), b"out_size"),
                        (dict(transform=1, ws=None), b"workspace"), (dict(transform=2, wsb=100), b"workspace"),
                        (dict(), b"packed"), (dict(transform=1), b"packed")]:    # no GPU here: nothing was ever packed
            assert call(**kw) != 0, kw
            assert msg in L.mi355_last_error(), (kw, L.mi355_last_error())
    finally:
        L.mi355_model_destroy(m)
        L.mi355_model_destroy(sw)


def test_workspace_queries_grow_with_batch_and_heights():
    L = _lib.lib()
    one, _ = _desc([(300, 400)])
    two, _ = _desc([(300, 400), (300, 400)])
    tall, _ = _desc([(900, 400)])
    q = lambda d, pad=0: L.mi355_resize_batch_workspace_bytes(_p(d), len(d), 224, 224, pad)
    assert 0 < q(one) < q(two)
    assert q(one) < q(tall)
    # pad mode: the source is the S x S square, S = 400 > 300
    assert q(one) < q(one, pad=1)
    # the temporary holds the rows the vertical pass reads, times out_w * 3 bytes, for every image
    assert q(two) >= 2 * 300 * 224 * 3
    f = lambda d, t: L.mi355_model_forward_images_workspace_bytes(_p(d), len(d), t, 224)
    assert f(one, 0) == 0                                          # "pad": fused into the stem, no workspace
    assert f(one, 1) >= 224 * 224 * 3 + q(one) and f(one, 1) < f(two, 1) and f(one, 1) < f(tall, 1)
    assert f(one, 2) > f(one, 1)
    bad, _ = _desc([(0, 5)])
    assert q(bad) == 0 and f(bad, 1) == 0
    assert L.mi355_resize_batch_workspace_bytes(None, 1, 224, 224, 0) == 0
