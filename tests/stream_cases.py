"""The table of stream cases: one ``stream_harness.Case`` per public GPU entry, at the smallest shapes that still take each
path (G = 300-400 rows, D = 70 - no multiple of 4 - and one D = 1536, Q = 37 and Q = 2 for the GEMV paths, k = 3 fused, k = 9
and k = 150 bitonic).  ``make(device)`` runs on the GPU only; the names, ``covers`` and ``syncs`` are plain data, so
tests/test_stream_cases_args.py checks on the CPU that every public entry has a case or a stated reason not to.

A (real) and B (decoy) inputs are both valid: the same shapes and dtypes, labels from one label set, ``exclude`` below the
row count, probe ids distinct and below ``nlist``, assignments below ``K``.  No NaN, no out-of-range index.
"""
from __future__ import annotations

import functools

import torch

from stream_harness import Case

G, D, Q, NLAB, NLIST = 400, 70, 37, 10, 8
BIG_D, BIG_G = 1536, 300
MODELS = ("efficientnet_b3a", "rexnet_150", "swin_base_patch4_window7_224", "swin_s3_base_224")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def randn(seed, *shape):
    return torch.randn(shape, generator=_gen(seed))


def randint(seed, hi, *shape):
    return torch.randint(0, hi, shape, generator=_gen(seed), dtype=torch.int64)


def u8(seed, *shape):
    return torch.randint(0, 256, shape, generator=_gen(seed), dtype=torch.uint8)


def pair(dev, **kinds):
    """A and B from ``name=(maker, *args)``: maker(seed, *args) with one seed for A and another for B."""
    A = {k: v[0](1000 + 7 * i, *v[1:]).to(dev) for i, (k, v) in enumerate(sorted(kinds.items()))}
    B = {k: v[0](5000 + 7 * i, *v[1:]).to(dev) for i, (k, v) in enumerate(sorted(kinds.items()))}
    return A, B


def _distinct(seed, hi, n, k):
    """(n, k) int64 rows of k DISTINCT values below hi."""
    g = _gen(seed)
    return torch.stack([torch.randperm(hi, generator=g)[:k] for _ in range(n)])


# ---------------------------------------------------------------------------------------------- shared stateful objects
@functools.lru_cache(maxsize=None)
def model(name):
    import imageretrievalresearch_amd as M
    return M.create_model(name, num_classes=0).to("cuda:0").eval()


@functools.lru_cache(maxsize=None)
def gallery(dtype, dim=D, rows=G):
    import imageretrievalresearch_amd as M
    g = M.Gallery(dim, "cuda:0", capacity=rows, dtype=dtype)
    g.add(randn(11, rows, dim).to("cuda:0"), randint(12, NLAB, rows).to("cuda:0"))
    torch.cuda.synchronize()
    return g


@functools.lru_cache(maxsize=None)
def int8_gallery():
    import imageretrievalresearch_amd as M
    g = M.Int8Gallery(D, "cuda:0", capacity=G)
    g.add(randn(11, G, D).to("cuda:0"), randint(12, NLAB, G).to("cuda:0"))
    torch.cuda.synchronize()
    return g


@functools.lru_cache(maxsize=None)
def whitening():
    import imageretrievalresearch_amd as M
    w = M.Whitening.fit(gallery(torch.float32), 32)
    torch.cuda.synchronize()
    return w


@functools.lru_cache(maxsize=None)
def ivf_index(dtype):
    ix = gallery(dtype).ivf(NLIST, iters=3, seed=0)
    torch.cuda.synchronize()
    return ix


CASES: list = []


def case(name, covers, syncs, control=True):
    def deco(make):
        CASES.append(Case(name, tuple(covers), make, syncs, control))
        return make
    return deco


def _queries(dev, dim=D, q=Q):
    return pair(dev, q=(randn, q, dim))


def _filtered(dev, rows=G, q=Q, dim=D):
    return pair(dev, q=(randn, q, dim), ql=(randint, NLAB, q), ex=(randint, rows, q))


# ---------------------------------------------------------------------------------------------- embed
def _images(dev, b):
    return pair(dev, x=(randn, b, 3, 224, 224))


for _name in MODELS:
    def _mk_forward(dev, _name=_name):
        m = model(_name)
        return (lambda i: m(i["x"])), *_images(dev, 2)

    def _mk_features(dev, _name=_name):
        m = model(_name)
        return (lambda i: m.forward_features(i["x"])), *_images(dev, 2)

    def _mk_u8(dev, _name=_name):
        m = model(_name)
        return (lambda i: m.forward_uint8(i["x"])), *pair(dev, x=(u8, 2, 224, 200, 3))

    def _mk_images_pad(dev, _name=_name):
        m = model(_name)
        return (lambda i: m.forward_images([i["a"], i["b"]], "pad")), *pair(dev, a=(u8, 224, 180, 3), b=(u8, 150, 224, 3))

    case(f"forward[{_name}]", ["Model.forward"], False)(_mk_forward)
    case(f"forward_features[{_name}]", ["Model.forward_features"], False)(_mk_features)
    case(f"forward_uint8[{_name}]", ["Model.forward_uint8"], False)(_mk_u8)
    case(f"forward_images_pad[{_name}]", ["Model.forward_images"], False)(_mk_images_pad)


def _option(m, key, value, fn):
    m.set_option(key, value)
    try:
        return fn()
    finally:
        m.set_option(key, 1 if key == "lanes" else 0)


@case("forward_lanes2_B64[efficientnet_b3a]", ["Model.forward", "Model.set_option"], False)
def _(dev):
    m = model("efficientnet_b3a")
    return (lambda i: _option(m, "lanes", 2, lambda: m(i["x"]))), *_images(dev, 64)


@case("forward_microbatch24_B64[efficientnet_b3a]", ["Model.forward", "Model.set_option"], False)
def _(dev):
    m = model("efficientnet_b3a")
    return (lambda i: _option(m, "microbatch", 24, lambda: m(i["x"]))), *_images(dev, 64)


@case("embed[efficientnet_b3a]", ["Model.embed"], False)
def _(dev):
    m = model("efficientnet_b3a")
    return (lambda i: m.embed(i["x"])), *_images(dev, 2)


for _mode in ("resize", "pad_resize"):
    # (the first call of a process on a source size uploads its coefficient table and waits for it: syncs=True)
    def _mk(dev, _mode=_mode):
        m = model("efficientnet_b3a")
        return ((lambda i: m.forward_images([i["a"], i["b"]], _mode)),
                *pair(dev, a=(u8, 97, 131, 3), b=(u8, 203, 77, 3)))
    case(f"forward_images_{_mode}[efficientnet_b3a]", ["Model.forward_images"], True)(_mk)


@case("forward_images_resize[swin_base_patch4_window7_224]", ["Model.forward_images"], True)
def _(dev):
    m = model("swin_base_patch4_window7_224")
    return (lambda i: m.forward_images([i["a"], i["b"]], "resize")), *pair(dev, a=(u8, 101, 67, 3), b=(u8, 59, 241, 3))


def _with_taps(m, fn):
    m.enable_taps(True)
    try:
        return fn()
    finally:
        m.enable_taps(False)


@case("taps[efficientnet_b3a]", ["Model.enable_taps", "Model.read_tap"], False)
def _(dev):
    m = model("efficientnet_b3a")
    return (lambda i: _with_taps(m, lambda: (m(i["x"]), m.read_tap("stem"), m.read_tap("blocks.5.1")))), *_images(dev, 2)


@case("run_between_taps[efficientnet_b3a]", ["Model.run_between_taps", "Model.read_tap"], False)
def _(dev):
    m = model("efficientnet_b3a")
    shape = _with_taps(m, lambda: (m(randn(3, 2, 3, 224, 224).to(dev)), m.read_tap("blocks.5.0").shape))[1]
    A, B = pair(dev, t=(lambda s, *sh: randn(s, *sh).bfloat16().float(), *shape))

    def op(i):
        return _with_taps(m, lambda: (m.run_between_taps("blocks.5.0", "blocks.5.1", i["t"]), m.read_tap("blocks.5.1"))[1])
    return op, A, B


@case("with_conv_input[efficientnet_b3a]", ["with_conv_input"], False)
def _(dev):
    import imageretrievalresearch_amd as M
    seq = M.models.with_conv_input(model("efficientnet_b3a")).to(dev).eval()
    return (lambda i: seq(i["x"])), *_images(dev, 2)


@case("forward_uint8_conv_input[efficientnet_b3a]", ["Model.forward_uint8", "with_conv_input"], False)
def _(dev):
    import imageretrievalresearch_amd as M
    m = model("efficientnet_b3a")
    seq = M.models.with_conv_input(m).to(dev).eval()
    return (lambda i: m.forward_uint8(i["x"], conv_input=seq[0])), *pair(dev, x=(u8, 2, 200, 224, 3))


@case("preprocess.resize", ["preprocess.resize"], True)
def _(dev):
    from imageretrievalresearch_amd import preprocess
    return (lambda i: preprocess.resize(i["a"], (224, 224))), *pair(dev, a=(u8, 93, 141, 3))


@case("resize_batch", ["resize_batch"], True)
def _(dev):
    import imageretrievalresearch_amd as M
    return (lambda i: M.resize_batch([i["a"], i["b"]], (224, 224))), *pair(dev, a=(u8, 83, 127, 3), b=(u8, 301, 55, 3))


@case("resize_batch_pad_packed", ["resize_batch", "pack_images"], True)
def _(dev):
    import imageretrievalresearch_amd as M
    return ((lambda i: M.resize_batch(M.pack_images([i["a"], i["b"]]), (64, 48), pad=True)),
            *pair(dev, a=(u8, 83, 127, 3), b=(u8, 301, 55, 3)))


@case("pack_images", ["pack_images"], False)
def _(dev):
    import imageretrievalresearch_amd as M
    return (lambda i: M.pack_images([i["a"], i["b"]])), *pair(dev, a=(u8, 33, 27, 3), b=(u8, 31, 55, 3))


@case("square_pad_normalize", ["preprocess.square_pad_normalize"], False)
def _(dev):
    from imageretrievalresearch_amd import preprocess
    return ((lambda i: preprocess.square_pad_normalize([i["a"], i["b"]])),
            *pair(dev, a=(u8, 224, 180, 3), b=(u8, 150, 224, 3)))


# ---------------------------------------------------------------------------------------------- rank functions
@case("l2_normalize_rows", ["l2_normalize_rows"], False)
def _(dev):
    import imageretrievalresearch_amd as M
    return (lambda i: M.l2_normalize_rows(i["q"])), *_queries(dev)


@case("synth_fill", ["synth_fill"], False, control=False)      # no device input: nothing for a control to read early
def _(dev):
    import imageretrievalresearch_amd as M
    return (lambda i: M.synth_fill(5000, 3, 1, dev)), {}, {}


@case("cosine_scores", ["cosine_scores"], False)
def _(dev):
    import imageretrievalresearch_amd as M
    return (lambda i: M.cosine_scores(i["q"], i["g"])), *pair(dev, q=(randn, Q, D), g=(randn, 300, D))


@case("cosine_scores_gemv_Q2", ["cosine_scores"], False)
def _(dev):
    import imageretrievalresearch_amd as M
    return (lambda i: M.cosine_scores(i["q"], i["g"])), *pair(dev, q=(randn, 2, D), g=(randn, 300, D))


for _tag, _q, _k, _dim, _rows in (("gemv_Q2_k3", 2, 3, D, 300), ("fused_k3", Q, 3, D, 300), ("k9", Q, 9, D, 300),
                                  ("bitonic_k150", Q, 150, D, 300), ("gemv_Q2_k150", 2, 150, D, 300),
                                  ("fused_k3_D1536", Q, 3, BIG_D, BIG_G)):
    def _mk(dev, _q=_q, _k=_k, _dim=_dim, _rows=_rows):
        import imageretrievalresearch_amd as M
        return (lambda i: M.cosine_topk(i["q"], i["g"], _k)), *pair(dev, q=(randn, _q, _dim), g=(randn, _rows, _dim))
    case(f"cosine_topk_{_tag}", ["cosine_topk"], False)(_mk)

for _tag, _q, _k, _mode in (("gemv_Q2_k3", 2, 3, "same"), ("fused_k3", Q, 3, "different"), ("bitonic_k150", Q, 150, "same")):
    def _mk(dev, _q=_q, _k=_k, _mode=_mode):
        import imageretrievalresearch_amd as M

        def op(i):
            return M.cosine_topk(i["q"], i["g"], _k, query_labels=i["ql"], gallery_labels=i["gl"], label_filter=_mode,
                                 exclude=i["ex"])
        return op, *pair(dev, q=(randn, _q, D), g=(randn, 300, D), ql=(randint, NLAB, _q), gl=(randint, NLAB, 300),
                         ex=(randint, 300, _q))
    case(f"cosine_topk_filtered_{_tag}", ["cosine_topk"], False)(_mk)


@case("PreparedGallery.search", ["PreparedGallery", "PreparedGallery.search"], False)
def _(dev):
    import imageretrievalresearch_amd as M

    def op(i):
        return M.PreparedGallery(M.l2_normalize_rows(i["g"])).search(i["q"], 3)
    return op, *pair(dev, q=(randn, Q, D), g=(randn, 300, D))


@case("topk", ["topk"], False)
def _(dev):
    import imageretrievalresearch_amd as M
    return (lambda i: (M.topk(i["s"], 9), M.topk(i["s"][0], 3), M.topk(i["s"], 150))), *pair(dev, s=(randn, Q, G))


@case("merge_topk", ["merge_topk"], False)
def _(dev):
    import imageretrievalresearch_amd as M
    return (lambda i: M.merge_topk(i["v"], i["i"], 9)), *pair(dev, v=(randn, Q, 40), i=(randint, G, Q, 40))


@case("pack_candidates", ["pack_candidates"], False)
def _(dev):
    from imageretrievalresearch_amd import rank
    return (lambda i: rank.pack_candidates(i["v"], i["i"], Q, 5, dev)), *pair(dev, v=(randn, Q, 3), i=(randint, G, Q, 3))


@case("merge_packed_topk", ["merge_packed_topk", "pack_candidates"], False)
def _(dev):
    from imageretrievalresearch_amd import rank
    off = torch.tensor([0, G], dtype=torch.int64, device=dev)

    def op(i):
        packed = torch.stack([rank.pack_candidates(i["v0"], i["i0"], Q, 5, dev), rank.pack_candidates(i["v1"], i["i1"], Q, 5, dev)])
        return rank.merge_packed_topk(packed, off, 5)
    return op, *pair(dev, v0=(randn, Q, 5), i0=(randint, G, Q, 5), v1=(randn, Q, 3), i1=(randint, G, Q, 3))


def _two(dev, b=Q):
    return pair(dev, a=(randn, b, D), b=(randn, b, D))


@case("pair_cosine", ["pair_cosine"], False)
def _(dev):
    import imageretrievalresearch_amd as M
    return (lambda i: M.pair_cosine(i["a"], i["b"])), *_two(dev)


@case("CosineSimilarity", ["CosineSimilarity"], False)
def _(dev):
    import imageretrievalresearch_amd as M
    cos = M.CosineSimilarity(dim=1, eps=1e-6)
    return (lambda i: (cos(i["a"], i["b"]), cos(i["a"][:1], i["b"]))), *_two(dev)


@case("ContrastiveLoss", ["ContrastiveLoss"], False)
def _(dev):
    import imageretrievalresearch_amd as M
    loss = M.ContrastiveLoss(0.5)
    return (lambda i: (loss(i["a"], i["b"], 1.0), loss(i["a"], i["b"], 0.0, mean=False))), *_two(dev)


@case("CosineEmbeddingLoss", ["CosineEmbeddingLoss"], False)
def _(dev):
    import imageretrievalresearch_amd as M
    loss = M.CosineEmbeddingLoss(0.5)
    return (lambda i: (loss(i["a"], i["b"], 1.0), loss(i["a"], i["b"], -1.0))), *_two(dev)


@case("validation_metrics", ["validation_metrics"], False)
def _(dev):
    import imageretrievalresearch_amd as M
    return ((lambda i: M.validation_metrics(i["a"], i["p"], i["n"], i["c"])),
            *pair(dev, a=(randn, Q, D), p=(randn, Q, D), n=(randn, Q, D), c=(randint, NLAB, Q)))


@case("hit_counts", ["hit_counts"], False)
def _(dev):
    import imageretrievalresearch_amd as M
    return ((lambda i: M.hit_counts(i["i"], i["qc"], i["gc"])),
            *pair(dev, i=(randint, G, Q, 3), qc=(randint, 3, Q), gc=(randint, 3, G)))


@case("distinct_class_topn", ["distinct_class_topn"], False)
def _(dev):
    import imageretrievalresearch_amd as M
    return ((lambda i: M.distinct_class_topn(i["i"], i["v"], i["gc"], 3)),
            *pair(dev, i=(randint, G, Q, 9), v=(randn, Q, 9), gc=(randint, NLAB, G)))


@case("retrieval_metrics", ["retrieval_metrics"], True)
def _(dev):
    import imageretrievalresearch_amd as M
    return ((lambda i: M.retrieval_metrics(i["a"], i["b"], i["c"])),
            *pair(dev, a=(randn, Q, D), b=(randn, Q, D), c=(randint, 4, Q)))


@case("retrieval_accuracy", ["retrieval_accuracy"], True)
def _(dev):
    import imageretrievalresearch_amd as M
    return ((lambda i: (M.retrieval_accuracy(i["q"], i["ql"]), M.retrieval_accuracy(i["q"], i["ql"], i["g"], i["gl"]))),
            *pair(dev, q=(randn, Q, D), ql=(randint, NLAB, Q), g=(randn, 300, D), gl=(randint, NLAB, 300)))


@case("roc_curve", ["roc_curve"], False)
def _(dev):
    import imageretrievalresearch_amd as M
    return ((lambda i: M.roc_curve(i["s"], i["a"])),
            *pair(dev, s=(lambda s, n: torch.rand(n, generator=_gen(s)), 500), a=(randint, 2, 500)))


@case("verification_roc", ["verification_roc"], False)
def _(dev):
    import imageretrievalresearch_amd as M
    return ((lambda i: (M.verification_roc(i["q"], i["ql"]), M.verification_roc(i["q"], i["ql"], i["g"], i["gl"]))),
            *pair(dev, q=(randn, Q, D), ql=(randint, NLAB, Q), g=(randn, 300, D), gl=(randint, NLAB, 300)))


@case("score_boosters", ["cos_sim_score_with_threshold", "cos_sim_score_booster"], False)
def _(dev):
    import imageretrievalresearch_amd as M

    def op(i):
        return (M.cos_sim_score_with_threshold(i["s"], 1e-6, 0.3, 0.5), M.cos_sim_score_booster(i["s"], 1e-6, 0.3, "for_pos"),
                M.cos_sim_score_booster(i["s"], 1e-6, 0.3, "for_neg"))
    return op, *pair(dev, s=(lambda s, n: torch.rand(n, generator=_gen(s)), 777))


@case("cosine_range", ["cosine_range"], True)
def _(dev):
    import imageretrievalresearch_amd as M
    return (lambda i: M.cosine_range(i["q"], i["g"], 0.1)), *pair(dev, q=(randn, Q, D), g=(randn, 300, D))


@case("positive_ranks", ["positive_ranks"], True)
def _(dev):
    import imageretrievalresearch_amd as M
    return ((lambda i: M.positive_ranks(i["q"], i["ql"], i["g"], i["gl"])),
            *pair(dev, q=(randn, Q, D), ql=(randint, NLAB, Q), g=(randn, 300, D), gl=(randint, NLAB, 300)))


@case("ranking_metrics", ["ranking_metrics"], True)
def _(dev):
    import imageretrievalresearch_amd as M
    return (lambda i: M.ranking_metrics(i["q"], i["ql"])), *pair(dev, q=(randn, 120, D), ql=(randint, NLAB, 120))


@case("expand_queries", ["expand_queries"], False)
def _(dev):
    import imageretrievalresearch_amd as M
    return (lambda i: M.expand_queries(i["q"], i["g"], 5, 3.0)), *pair(dev, q=(randn, Q, D), g=(randn, 300, D))


@case("k_reciprocal_rerank", ["k_reciprocal_rerank"], True)
def _(dev):
    import imageretrievalresearch_amd as M
    return ((lambda i: M.k_reciprocal_rerank(i["q"], i["g"], 5, k1=6, k2=3, shortlist=20)),
            *pair(dev, q=(randn, Q, D), g=(randn, 300, D)))


# ---------------------------------------------------------------------------------------------- resident objects
for _dt, _tag in ((torch.float32, "f32"), (torch.float16, "f16")):
    def _mk_add(dev, _dt=_dt):
        import imageretrievalresearch_amd as M

        def op(i):      # two adds, the second one grows the buffer
            g = M.Gallery(D, dev, capacity=200, dtype=_dt).add(i["r"][:200], i["l"][:200]).add(i["r"][200:], i["l"][200:])
            return g.data, g.labels
        return op, *pair(dev, r=(randn, 300, D), l=(randint, NLAB, 300))

    def _mk_search(dev, _dt=_dt):
        g = gallery(_dt)
        return (lambda i: (g.search(i["q"], 3), g.search(i["q"], 9), g.search(i["q"], 150), g.search(i["q"][:2], 3))), *_queries(dev)

    def _mk_search_filtered(dev, _dt=_dt):
        g = gallery(_dt)

        def op(i):
            return (g.search(i["q"], 3, query_labels=i["ql"], label_filter="same", exclude=i["ex"]),
                    g.search(i["q"], 150, query_labels=i["ql"], label_filter="different"),
                    g.search(i["q"][:2], 3, exclude=i["ex"][:2]))
        return op, *_filtered(dev)

    def _mk_search_qe(dev, _dt=_dt):
        g = gallery(_dt)
        return (lambda i: (g.search(i["q"], 3, qe=(5, 3.0)), g.expand_queries(i["q"], 5, 2.0))), *_queries(dev)

    def _mk_augmented(dev, _dt=_dt):
        import imageretrievalresearch_amd as M

        def op(i):
            return M.Gallery(D, dev, capacity=300, dtype=_dt).add(i["r"]).augmented(5, 3.0, block=128).data
        return op, *pair(dev, r=(randn, 300, D))

    def _mk_knn(dev, _dt=_dt):
        import imageretrievalresearch_amd as M

        def op(i):
            g = M.Gallery(D, dev, capacity=300, dtype=_dt).add(i["r"])
            ix = g.rerank_index(6, 3)
            return g.knn_graph(6), ix.tau, ix.V, ix.V2, ix.nbytes
        return op, *pair(dev, r=(randn, 300, D))

    def _mk_rerank(dev, _dt=_dt):
        g = gallery(_dt)
        g.rerank_index(6, 3)
        return (lambda i: (g.rerank(i["q"], 5, k1=6, k2=3, shortlist=20), g.rerank(i["q"][:2], 5, k1=6, k2=3, shortlist=20,
                                                                                  exclude=i["ex"][:2]))), *_filtered(dev)

    def _mk_moments(dev, _dt=_dt):
        import imageretrievalresearch_amd as M
        return (lambda i: M.Gallery(D, dev, capacity=300, dtype=_dt).add(i["r"]).moments()), *pair(dev, r=(randn, 300, D))

    def _mk_whitened(dev, _dt=_dt):
        import imageretrievalresearch_amd as M
        w = whitening()
        return (lambda i: M.Gallery(D, dev, capacity=300, dtype=_dt).add(i["r"]).whitened(w).data), *pair(dev, r=(randn, 300, D))

    def _mk_range(dev, _dt=_dt):
        g = gallery(_dt)
        return ((lambda i: (g.range_search(i["q"], 0.1), g.range_search(i["q"], 0.0, query_labels=i["ql"], label_filter="same",
                                                                       exclude=i["ex"]))), *_filtered(dev))

    def _mk_roc(dev, _dt=_dt):
        g = gallery(_dt)
        return (lambda i: g.verification_roc(i["q"], i["ql"], exclude=i["ex"])), *_filtered(dev)

    def _mk_ranking(dev, _dt=_dt):
        g = gallery(_dt)
        return (lambda i: g.ranking_metrics(i["q"], i["ql"], exclude=i["ex"])), *_filtered(dev)

    def _mk_kmeans(dev, _dt=_dt):
        import imageretrievalresearch_amd as M

        def op(i):
            g = M.Gallery(D, dev, capacity=300, dtype=_dt).add(i["r"], i["l"])
            return g.kmeans(NLIST, iters=3, seed=1), g.clustering_metrics(iters=2)
        return op, *pair(dev, r=(randn, 300, D), l=(randint, NLAB, 300))

    def _mk_ivf_build(dev, _dt=_dt):
        import imageretrievalresearch_amd as M

        def op(i):
            g = M.Gallery(D, dev, capacity=300, dtype=_dt).add(i["r"][:250])
            ix = g.ivf(NLIST, iters=2, seed=0)
            g.add(i["r"][250:])
            ix.update()
            return ix.centroids, ix.offsets, ix.order, ix.counts, ix.assignments, ix.search(i["r"][:5], 3, 2), ix.nbytes, ix.stale
        return op, *pair(dev, r=(randn, 300, D))

    def _mk_ivf_search(dev, _dt=_dt):
        ix = ivf_index(_dt)

        def op(i):
            return (ix.search(i["q"], 3, 3), ix.probe(i["q"], 3), ix.search(i["q"], 9, probes=i["p"]),
                    ix.search(i["q"], 3, 2, query_labels=i["ql"], label_filter="same", exclude=i["ex"]), ix.recall(i["q"], 3, 4))
        A, B = _filtered(dev)
        A["p"], B["p"] = _distinct(31, NLIST, Q, 3).to(dev), _distinct(32, NLIST, Q, 3).to(dev)
        return op, A, B

    case(f"Gallery.add[{_tag}]", ["Gallery", "Gallery.add", "Gallery.data"], False)(_mk_add)
    case(f"Gallery.search[{_tag}]", ["Gallery.search"], False)(_mk_search)
    case(f"Gallery.search_filtered[{_tag}]", ["Gallery.search"], False)(_mk_search_filtered)
    case(f"Gallery.search_qe[{_tag}]", ["Gallery.search", "Gallery.expand_queries"], False)(_mk_search_qe)
    case(f"Gallery.augmented[{_tag}]", ["Gallery.augmented"], False)(_mk_augmented)
    case(f"Gallery.knn_graph[{_tag}]", ["Gallery.knn_graph", "Gallery.rerank_index", "RerankIndex", "RerankIndex.nbytes"], True)(_mk_knn)
    case(f"Gallery.rerank[{_tag}]", ["Gallery.rerank"], True)(_mk_rerank)
    case(f"Gallery.moments[{_tag}]", ["Gallery.moments"], False)(_mk_moments)
    case(f"Gallery.whitened[{_tag}]", ["Gallery.whitened"], False)(_mk_whitened)
    case(f"Gallery.range_search[{_tag}]", ["Gallery.range_search"], True)(_mk_range)
    case(f"Gallery.verification_roc[{_tag}]", ["Gallery.verification_roc"], False)(_mk_roc)
    case(f"Gallery.ranking_metrics[{_tag}]", ["Gallery.ranking_metrics"], True)(_mk_ranking)
    case(f"Gallery.kmeans[{_tag}]", ["Gallery.kmeans", "Gallery.clustering_metrics"], True)(_mk_kmeans)
    case(f"Gallery.ivf[{_tag}]", ["Gallery.ivf", "IVFIndex", "IVFIndex.build", "IVFIndex.update", "IVFIndex.nbytes",
                                  "IVFIndex.stale"], True)(_mk_ivf_build)
    case(f"IVFIndex.search[{_tag}]", ["IVFIndex.search", "IVFIndex.probe", "IVFIndex.recall"], True)(_mk_ivf_search)


@case("Gallery.prepare", ["Gallery.prepare", "Gallery.nbytes"], False)
def _(dev):
    import imageretrievalresearch_amd as M

    def op(i):
        g = M.Gallery(D, dev, capacity=300).add(i["g"]).prepare()
        return g.search(i["q"], 3), g.search(i["q"], 9), g.nbytes
    return op, *pair(dev, q=(randn, Q, D), g=(randn, 300, D))


@case("Gallery.search_D1536", ["Gallery.search"], False)
def _(dev):
    g = gallery(torch.float32, BIG_D, BIG_G)
    return (lambda i: (g.search(i["q"], 3), g.search(i["q"][:2], 3))), *_queries(dev, BIG_D)


@case("Gallery.quantized", ["Gallery.quantized"], False)
def _(dev):
    import imageretrievalresearch_amd as M

    def op(i):
        z = M.Gallery(D, dev, capacity=300).add(i["r"], i["l"]).quantized()
        return z.codes, z.scales, z.labels
    return op, *pair(dev, r=(randn, 300, D), l=(randint, NLAB, 300))


@case("Int8Gallery.add", ["Int8Gallery", "Int8Gallery.add", "Int8Gallery.codes", "Int8Gallery.scales", "Int8Gallery.dequantized",
                          "Int8Gallery.nbytes"], False)
def _(dev):
    import imageretrievalresearch_amd as M

    def op(i):
        g = M.Int8Gallery(D, dev, capacity=200).add(i["r"][:200], i["l"][:200]).add(i["r"][200:], i["l"][200:])
        return g.codes, g.scales, g.labels, g.dequantized(), g.nbytes
    return op, *pair(dev, r=(randn, 300, D), l=(randint, NLAB, 300))


@case("Int8Gallery.search", ["Int8Gallery.search"], False)
def _(dev):
    g = int8_gallery()
    return (lambda i: (g.search(i["q"], 3), g.search(i["q"], 150), g.search(i["q"][:2], 3))), *_queries(dev)


@case("Int8Gallery.search_filtered", ["Int8Gallery.search"], False)
def _(dev):
    g = int8_gallery()

    def op(i):
        return (g.search(i["q"], 3, query_labels=i["ql"], label_filter="same", exclude=i["ex"]),
                g.search(i["q"][:2], 9, query_labels=i["ql"][:2], label_filter="different"))
    return op, *_filtered(dev)


@case("Int8Gallery.range_search", ["Int8Gallery.range_search"], True)
def _(dev):
    g = int8_gallery()
    return (lambda i: g.range_search(i["q"], 0.1)), *_queries(dev)


@case("Int8Gallery.recall", ["Int8Gallery.recall"], True)
def _(dev):
    g, exact = int8_gallery(), gallery(torch.float32)
    return (lambda i: g.recall(i["q"], 150, exact)), *_queries(dev)


@case("Whitening.fit", ["Whitening", "Whitening.fit", "Whitening.to"], True)
def _(dev):
    import imageretrievalresearch_amd as M

    def op(i):
        w = M.Whitening.fit(i["r"], 16, block=128)
        return w.matrix, w.bias, w.mean
    return op, *pair(dev, r=(randn, 300, D))


@case("Whitening.transform", ["Whitening.transform"], False)
def _(dev):
    w = whitening()
    return (lambda i: (w.transform(i["q"]), w.transform(i["q"], normalize_output=False))), *_queries(dev)


@case("embedding_moments_out", ["embedding_moments"], False)
def _(dev):
    import imageretrievalresearch_amd as M

    def op(i):
        m = M.embedding_moments(i["a"], normalize=True)
        return M.embedding_moments(i["b"], normalize=True, out=m)
    return op, *_two(dev, 150)


def _assign_inputs(dev):
    return pair(dev, r=(randn, 300, D), c=(randn, NLIST, D), a=(randint, NLIST, 300), l=(randint, NLAB, 300))


@case("assign_clusters", ["assign_clusters"], False)
def _(dev):
    import imageretrievalresearch_amd as M
    return (lambda i: M.assign_clusters(i["r"], i["c"])), *_assign_inputs(dev)


@case("update_centroids", ["update_centroids"], True)
def _(dev):
    import imageretrievalresearch_amd as M
    return (lambda i: M.update_centroids(i["r"], i["a"], NLIST, i["c"])), *_assign_inputs(dev)


@case("cluster_members", ["cluster_members"], True)
def _(dev):
    import imageretrievalresearch_amd as M
    return (lambda i: M.cluster_members(i["a"], NLIST)), *_assign_inputs(dev)


@case("contingency", ["contingency", "clustering_metrics"], True)
def _(dev):
    import imageretrievalresearch_amd as M
    return (lambda i: (M.contingency(i["a"], i["l"]), M.clustering_metrics(i["a"], i["l"]))), *_assign_inputs(dev)


@case("spherical_kmeans", ["spherical_kmeans"], True)
def _(dev):
    import imageretrievalresearch_amd as M
    return (lambda i: M.spherical_kmeans(i["r"], NLIST, iters=3, init=i["c"])), *_assign_inputs(dev)


@case("ShardedGallery.search", ["ShardedGallery", "ShardedGallery.search"], False)
def _(dev):
    import imageretrievalresearch_amd as M
    sh = M.ShardedGallery(randn(11, G, D).to(dev))
    return (lambda i: (sh.search(i["q"], 3), sh.search(i["q"], 150))), *_queries(dev)


@case("ShardedGallery.one_rank", ["ShardedGallery.search", "ShardedGallery.range_search", "ShardedGallery.verification_roc",
                                 "ShardedGallery.fit_whitening", "ShardedGallery.whitened"], True)
def _(dev):
    import imageretrievalresearch_amd as M

    def op(i):          # no process group: every method takes its one-rank path, which makes no collective call
        sh = M.ShardedGallery(i["r"], labels=i["l"])
        w = sh.fit_whitening(16)
        return (sh.search(i["q"], 3, query_labels=i["ql"], label_filter="same", exclude=i["ex"]), sh.search(i["q"], 3, qe=(5, 3.0)),
                sh.range_search(i["q"], 0.1), sh.verification_roc(i["q"], i["ql"], exclude=i["ex"]), w.matrix, w.bias,
                sh.whitened(w).local)
    return op, *pair(dev, r=(randn, 300, D), l=(randint, NLAB, 300), q=(randn, Q, D), ql=(randint, NLAB, Q), ex=(randint, 300, Q))


# ---------------------------------------------------------------------------------------------- what has no case, and why
HOST_ONLY = {
    "MI355Error": "exception type",
    "Moments": "NamedTuple result type",
    "KMeansResult": "NamedTuple result type",
    "PositiveRanks": "NamedTuple result type",
    "create_model": "builds the host-side parameter table; the first forward packs the weights",
    "list_models": "list of names",
    "load_checkpoint": "checkpoint helper: reads a file into host tensors",
    "strip_lightning_prefix": "checkpoint helper: renames state-dict keys",
    "clustering_metrics_from_table": "host float64 half of clustering_metrics, needs no GPU",
    "Whitening.from_moments": "host float64 eigen-decomposition, needs no GPU",
    "Whitening.state_dict": "copies the fitted tensors to the host",
    "Whitening.load_state_dict": "host tensors in; the move to a device is Whitening.to",
    "PreparedGallery.supports": "static predicate on (Q, k)",
    "Model.traffic": "host-side byte / MAC model",
    "Model.profile_read": "reads the host-side timing table",
    "Model.profile_ops": "reads the host-side timing table",
    "Model.plan": "resolves a launch plan on the host",
    "Model.block_stamps": "diagnostic read-back that synchronises the whole device by design; launches nothing",
    "Model.reset_parameters": "host-side seeded init of the nn.Parameters",
    "Model.load_state_dict": "nn.Module state loading; the next forward packs",
    "Model.mark_dirty": "sets a flag",
    "ShardedGallery.offset": "property: the first global row of this rank's shard",
    "ShardedGallery.prepared": "property: the shard's planes or None",
    "ShardedGallery.my_slice": "host arithmetic on the rank",
}

# The collective paths of ShardedGallery (world size > 1: the all-gathers and all-reduces between the shards) need a process
# group and are out of scope here; every method's one-rank path has a case above.  An entry that can ONLY run inside a
# group belongs here, with its reason.
NEEDS_PROCESS_GROUP: dict = {}

# The entries that read something back to the host (their cases are declared syncs=True); INTEGRATION.md's "Streams" section
# names every one of them.  Everything else with a case returns while its work is still queued.
SYNCING = (
    "cosine_range", "Gallery.range_search", "Int8Gallery.range_search",                       # each query block's hit count
    "positive_ranks", "ranking_metrics", "Gallery.ranking_metrics",                           # the range pass and the offsets
    "retrieval_accuracy", "retrieval_metrics",                                                # max R_q / the returned floats
    "spherical_kmeans", "Gallery.kmeans", "Gallery.clustering_metrics", "clustering_metrics",  # convergence test, objective
    "contingency", "cluster_members", "update_centroids",                                     # the out-of-range flag
    "Gallery.ivf", "IVFIndex.build", "IVFIndex.update", "IVFIndex.search", "IVFIndex.recall",   # list lengths, the scan's flags
    "Int8Gallery.recall",                                                                     # returns a float
    "Whitening.fit",                                                                          # moments to the host eigensolver
    "Gallery.rerank_index", "Gallery.rerank", "k_reciprocal_rerank",                          # sizes of the sparse rows
    "resize_batch", "preprocess.resize", "Model.forward_images",                              # a first-seen source size
    "ShardedGallery.range_search", "ShardedGallery.fit_whitening",                            # as cosine_range / Whitening.fit
)
# In SYNCING for one of its modes only, so it also has syncs=False cases.
SOMETIMES_ASYNC = {"Model.forward_images": 'transform="pad" resizes nothing; the resize modes wait only for a first-seen size'}
