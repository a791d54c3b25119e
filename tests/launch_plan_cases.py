"""The cases of tests/test_launch_plan_args.py and what is collected for each, shared with the recording script
tests/golden/make_launch_plan_golden.py.  Everything here is host-only: model tables, the launch plan and the traffic
model need neither packed weights nor a GPU."""
import ctypes as C
import itertools

MODELS = ["efficientnet_b3a", "rexnet_150", "rexnet_200", "swin_base_patch4_window7_224", "swin_s3_base_224"]
# (whole batch, chunk).  20 / 21 straddle the LayerNorm fold's 1024-row edge at 7x7 tokens, 95 / 96 fuse_block_min_batch.
BATCHES = [(1, 1), (20, 20), (21, 21), (95, 95), (96, 96), (256, 256), (256, 128), (96, 48)]
SIZES_CONV = [(224, 224), (32, 32), (225, 231), (256, 320)]
SIZES_SWIN = [(224, 224)]
# the defaults, then each option alone; fuse_block_min_batch=1 goes with a batch of 2
OPTIONS = [None, ("fuse", 0), ("fuse_block", 0), ("fuse_block_min_batch", 1), ("fuse_band", 0), ("fuse_band", 1),
           ("fuse_sweep", 0), ("fuse_ln", 0), ("fuse_head_gap", 0)]
HOW = ["op", "fused_late", "sweep", "band", "block", "head_gap", "ln_stats"]   # MI355_PLAN_* of include/mi355_retrieval.h
MAX = 1024


def sizes(model):
    return SIZES_SWIN if model.startswith("swin") else SIZES_CONV


def batches(opt):
    return [(2, 2)] if opt == ("fuse_block_min_batch", 1) else BATCHES


def opt_name(opt):
    return "defaults" if opt is None else f"{opt[0]}={opt[1]}"


def bind(L, plan=True):
    """argtypes of the entries used here, for a library loaded with plain ctypes.CDLL"""
    vp, i, dp = C.c_void_p, C.c_int, C.POINTER(C.c_double)
    L.mi355_last_error.restype = C.c_char_p
    L.mi355_model_create.argtypes = [C.c_char_p, i, C.POINTER(vp)]
    L.mi355_model_destroy.argtypes = [vp]
    L.mi355_model_destroy.restype = None
    L.mi355_model_set_option.argtypes = [vp, C.c_char_p, C.c_int64]
    L.mi355_model_traffic_kinds.argtypes = [vp, i, i, i, dp, dp, i]
    L.mi355_model_profile_ops.argtypes = [vp, i, i, i, i, dp, dp, C.POINTER(i), C.c_char_p, i]
    if plan:
        ip = C.POINTER(i)
        L.mi355_model_plan.argtypes = [vp, i, i, i, i, i, i, ip, ip, ip, C.POINTER(C.c_size_t)]
    return L


def _model(L, name, opt):
    h = C.c_void_p()
    assert L.mi355_model_create(name.encode(), 0, C.byref(h)) == 0, L.mi355_last_error()
    if opt is not None:
        assert L.mi355_model_set_option(h, opt[0].encode(), opt[1]) == 0, L.mi355_last_error()
    return h


def _exact_int(v):
    assert v == int(v), v
    return int(v)


def collect_plans(L, name):
    """{"model|B|chunk|HxW|option|kind": (first_op[], n_ops[], how[], arena_bytes)}"""
    out = {}
    fo, no, hw = (C.c_int * MAX)(), (C.c_int * MAX)(), (C.c_int * MAX)()
    for opt in OPTIONS:
        h = _model(L, name, opt)
        for B, nb in batches(opt):
            for H, W in sizes(name):
                for pooled in (0, 1):
                    arena = C.c_size_t(0)
                    n = L.mi355_model_plan(h, B, nb, H, W, pooled, MAX, fo, no, hw, C.byref(arena))
                    assert 0 < n <= MAX, (n, L.mi355_last_error())
                    key = f"{name}|{B}|{nb}|{H}x{W}|{opt_name(opt)}|{'pooled' if pooled else 'features'}"
                    out[key] = (list(fo[:n]), list(no[:n]), list(hw[:n]), int(arena.value))
        L.mi355_model_destroy(h)
    return out


def collect_traffic(L, name):
    """{"model|B|HxW|option": bytes_by_kind[8] + macs_by_kind[8]}, whole numbers below 2^53"""
    out = {}
    by, mc = (C.c_double * 8)(), (C.c_double * 8)()
    for opt in OPTIONS:
        h = _model(L, name, opt)
        for B in sorted({b for b, _ in batches(opt)}):
            for H, W in sizes(name):
                assert L.mi355_model_traffic_kinds(h, B, H, W, by, mc, 8) == 0, L.mi355_last_error()
                out[f"{name}|{B}|{H}x{W}|{opt_name(opt)}"] = [_exact_int(v) for v in list(by) + list(mc)]
        L.mi355_model_destroy(h)
    return out


def collect_profile_ops(L, name):
    """{"model|B|HxW": (labels[], kinds[], bytes[])}; the per-op table does not depend on the options"""
    out = {}
    ms, by, kd = (C.c_double * MAX)(), (C.c_double * MAX)(), (C.c_int * MAX)()
    lab = C.create_string_buffer(MAX * 64)
    h = _model(L, name, None)
    for B in sorted({b for opt in OPTIONS for b, _ in batches(opt)}):
        for H, W in sizes(name):
            n = L.mi355_model_profile_ops(h, B, H, W, MAX, ms, by, kd, lab, 64)
            assert 0 < n <= MAX, (n, L.mi355_last_error())
            labels = [lab.raw[i * 64:(i + 1) * 64].split(b"\0")[0].decode() for i in range(n)]
            out[f"{name}|{B}|{H}x{W}"] = (labels, list(kd[:n]), [_exact_int(v) for v in by[:n]])
    L.mi355_model_destroy(h)
    return out


# ---- the golden file: every list is stored once in "lists" and referred to by its index
def encode_steps(first_op, n_ops, how):
    """steps that tile the ops in order are given by (n_ops, how) alone: two characters a step"""
    pos = 0
    for f, n in zip(first_op, n_ops):
        assert f == pos and 1 <= n <= 9, (f, pos, n)
        pos += n
    return "".join(f"{n}{h}" for n, h in zip(n_ops, how))


def decode_steps(s):
    n_ops = [int(c) for c in s[0::2]]
    how = [int(c) for c in s[1::2]]
    first_op = [0] + list(itertools.accumulate(n_ops))[:-1]
    return first_op, n_ops, how
