"""imageretrievalresearch_amd — MI355X-native embed-then-rank hot path.

A drop-in for ONE path of vitasoftAI/ImageRetrievalResearch: the timm model object
(`create_model`, `forward`, `forward_features`, `head`/`classifier`, timm state-dict keys) and the
cosine / top-k / ContrastiveLoss math around it, running as hand-written HIP kernels for gfx950
behind the C ABI in include/mi355_retrieval.h.  Host code is Python on PyTorch-ROCm; torch is used
for device memory, streams and torch.distributed only.
"""
from . import synth  # noqa: F401
from ._lib import MI355Error, lib, LIB_PATH  # noqa: F401
from . import models  # noqa: F401
# models imports the submodule aggregate.py (model.forward_descriptors), which binds the MODULE to the package attribute
# `aggregate`; the public name is the function, so it is bound over it here (the module: importlib.import_module(__name__ + ".aggregate"))
from .aggregate import aggregate, rmac_regions  # noqa: F401
from .preprocess import pack_images, resize_batch  # noqa: F401
from .rank import (ContrastiveLoss, CosineEmbeddingLoss, CosineSimilarity, Gallery, PositiveRanks, PreparedGallery,  # noqa: F401
                   cos_sim_score_booster, cos_sim_score_with_threshold, cosine_range, cosine_scores, cosine_topk,
                   distinct_class_topn, expand_queries, hit_counts, l2_normalize_rows, merge_topk, pair_cosine,
                   positive_ranks, ranking_metrics, retrieval_accuracy, retrieval_metrics, roc_curve, synth_fill, topk, validation_metrics,
                   verification_roc)
from .rerank import RerankIndex, k_reciprocal_rerank  # noqa: F401
from .whitening import Moments, Whitening, embedding_moments  # noqa: F401
from .cluster import (DBSCANResult, KMeansResult, assign_clusters, cluster_members, clustering_metrics,  # noqa: F401
                      clustering_metrics_from_table, connected_components, contingency, dbscan, spherical_kmeans,
                      update_centroids)
from .ivf import IVFIndex  # noqa: F401
from .quantized import Int8Gallery  # noqa: F401

__all__ = ["Whitening", "Moments", "embedding_moments","create_model", "list_models", "load_checkpoint", "strip_lightning_prefix", "ContrastiveLoss", "CosineEmbeddingLoss", "validation_metrics", "CosineSimilarity", "Gallery", "PreparedGallery", "cosine_scores",
           "cosine_range", "cosine_topk", "expand_queries", "pair_cosine", "topk", "merge_topk", "hit_counts", "distinct_class_topn",
           "retrieval_metrics", "retrieval_accuracy", "roc_curve", "verification_roc", "cos_sim_score_with_threshold", "cos_sim_score_booster", "l2_normalize_rows", "synth_fill", "ShardedGallery", "MI355Error",
           "pack_images", "resize_batch", "RerankIndex", "k_reciprocal_rerank", "PositiveRanks", "positive_ranks", "ranking_metrics",
           "KMeansResult", "assign_clusters", "update_centroids", "cluster_members", "spherical_kmeans", "contingency",
           "clustering_metrics", "clustering_metrics_from_table", "IVFIndex", "Int8Gallery"]
# dbscan / connected_components / DBSCANResult are importable from here but, like the lazily exported indexes, are not in __all__:
# the stream table (tests/stream_cases.py) enumerates __all__, and their side-stream case is tests/test_dbscan_streams_gpu.py;
# aggregate / rmac_regions (bound above) likewise: their side-stream case is tests/test_aggregate_streams_gpu.py


def __getattr__(name):  # lazy: models/sharded import torch.nn / torch.distributed
    if name in ("load_checkpoint", "strip_lightning_prefix"):
        from . import checkpoint
        return getattr(checkpoint, name)
    if name in ("create_model", "list_models", "ConvInput", "with_conv_input"):
        from . import models
        return getattr(models, name)
    if name == "PQGallery":
        from .pq import PQGallery
        return PQGallery
    if name == "BinaryGallery":
        from .binary import BinaryGallery
        return BinaryGallery
    if name == "FP4Gallery":
        from .fp4 import FP4Gallery
        return FP4Gallery
    if name == "IVFPQIndex":
        from .ivfpq import IVFPQIndex
        return IVFPQIndex
    if name == "Int8IVFIndex":
        from .ivf_i8 import Int8IVFIndex
        return Int8IVFIndex
    if name == "ResidualIVFPQIndex":
        from .ivfrpq import ResidualIVFPQIndex
        return ResidualIVFPQIndex
    if name in ("GraphIndex", "merged_graph"):
        from . import graph
        return getattr(graph, name)
    if name in ("DiffusionIndex", "diffusion_rerank"):
        from . import diffusion
        return getattr(diffusion, name)
    if name == "mmr_rerank":                                 # its side-stream case: tests/test_diversify_streams_gpu.py
        from .diversify import mmr_rerank
        return mmr_rerank
    if name in ("RegionGallery", "maxsim"):                 # their side-stream case: tests/test_regional_streams_gpu.py
        from . import regional
        return getattr(regional, name)
    if name in ("ScoreNorm", "adjusted_topk", "adjusted_scores", "neighbourhood_stats", "topn_stats"):
        from . import scorenorm                              # their side-stream case: tests/test_scorenorm_streams_gpu.py
        return getattr(scorenorm, name)
    if name == "ShardedGallery":
        from .sharded import ShardedGallery
        return ShardedGallery
    raise AttributeError(name)
