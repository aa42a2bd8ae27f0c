"""ssg_amd -- MI355X-native pseudo-label grouping for Self-Similarity Grouping.

One hot path: ResNet-50 embedding of the target set -> N x N
k-reciprocal re-rank distance -> epsilon rule -> DBSCAN, behind the reference's Python call
surface.  Compute = hand-written HIP kernels in csrc/ behind the C ABI of include/ssg_hip.h;
this package is the thin host-side mirror of the reference interface.
"""
from . import _lib  # noqa: F401
from ._lib import SSGError, available  # noqa: F401

__all__ = ["re_ranking", "re_ranking_device", "DBSCAN", "AffinityPropagation", "eps_rule", "eps_rule_dbscan", "compute_dist", "generate_selflabel", "SSGError", "available"]


def __getattr__(name):   # lazy: torch import only when the compute surface is touched
    if name in ("re_ranking", "re_ranking_device", "re_ranking_init", "re_ranking_init_device", "re_ranking_init_dist", "DistHandle", "ReRankNaNError"):
        from . import rerank
        return getattr(rerank, name)
    if name in ("estimate_label_device", "dissimilarity_from_dist", "nearest_labelled", "select_top", "EUGMixin", "updata_lable"):
        from . import eug
        return getattr(eug, name)
    if name == "generate_selflabel_semi":
        from . import semitraining
        return semitraining.generate_selflabel
    if name in ("DBSCAN", "AffinityPropagation", "eps_rule", "eps_rule_dbscan", "as_handle"):
        from . import cluster
        return getattr(cluster, name)
    if name in ("OPTICS", "compute_optics_graph", "cluster_optics_dbscan", "cluster_optics_xi"):
        from . import optics
        return getattr(optics, name)
    if name == "HDBSCAN":
        from . import hdbscan
        return hdbscan.HDBSCAN
    if name == "AgglomerativeClustering":
        from . import agglomerative
        return agglomerative.AgglomerativeClustering
    if name in ("silhouette_samples", "silhouette_score", "silhouette_many"):
        from . import silhouette
        return getattr(silhouette, name)
    if name in ("compute_dist", "generate_selflabel", "generate_selflabel_affinity", "generate_selflabel_optics", "generate_selflabel_hdbscan",
                "generate_selflabel_agglomerative", "generate_selflabel_sweep", "select_labeled", "generate_dataset"):
        from . import selftraining
        return getattr(selftraining, name)
    if name in ("extract_features", "extract_embeddings", "extract_cnn_feature", "fliplr", "pairwise_distance", "pairwise_distance_device",
                "TensorBatchLoader"):
        from . import evaluators
        return getattr(evaluators, name)
    if name in ("re_ranking_plain", "re_ranking_plain_device"):
        from . import rerank_plain
        return rerank_plain.re_ranking if name == "re_ranking_plain" else rerank_plain.re_ranking_plain_device
    if name in ("re_ranking_hausdorff", "re_ranking_hausdorff_device"):
        from . import rerank_hausdorff
        return rerank_hausdorff.re_ranking if name == "re_ranking_hausdorff" else rerank_hausdorff.re_ranking_hausdorff_device
    if name in ("cmc", "mean_ap", "evaluate_all", "evaluate_same_cams_all", "Evaluator", "single_shot_ranks", "RankNaNError"):
        from . import ranking
        return getattr(ranking, name)
    if name in ("get_metric", "KISSME", "Euclidean", "validate_cov_matrix"):       # reid/metric_learning/ (the two in-tree learners)
        from . import metric_learning
        return getattr(metric_learning, name)
    if name == "DistanceMetric":
        from . import dist_metric
        return dist_metric.DistanceMetric
    if name in ("find_metric_threshold", "cal_classification_error", "findMetricThreshold_MPI", "CalClassificationError_MPI", "VerificationResult"):
        from . import verification
        return getattr(verification, name)
    if name in ("Preprocessor", "GpuBatchLoader", "preprocess_batch"):
        from . import preprocessor
        return getattr(preprocessor, name)
    if name == "decode_jpeg_batch":
        from . import jpeg
        return jpeg.decode_batch
    if name == "triplet_pairwise_dist":
        from . import triplet
        return triplet.pairwise_dist
    if name == "TripletLoss":
        from . import triplet
        return triplet.TripletLoss
    if name in ("GpuTrainLoader", "TrainTransform", "generate_dataloader"):
        from . import trainloader
        return getattr(trainloader, name)
    if name in ("ClusterAssignment", "target_distribution", "kl_loss", "use_device_assignment", "soft_assignment"):
        from . import dce
        return getattr(dce, name)
    if name in ("batch_norm_train", "BatchNorm1d", "BatchNorm2d", "use_device_batchnorm"):
        from . import batchnorm
        return getattr(batchnorm, name)
    if name in ("conv2d_train", "Conv2d", "use_device_conv"):
        from . import conv
        return getattr(conv, name)
    if name in ("conv2d_train_strided", "StridedConv2d", "max_pool2d_train", "MaxPool2d", "use_device_maxpool"):
        from . import conv_strided
        return getattr(conv_strided, name)
    if name in ("stripe_pool_train", "linear_train", "Linear", "DeviceHeadMixin", "use_device_head"):
        from . import head
        return getattr(head, name)
    if name in ("SGD", "use_device_sgd"):
        from . import sgd
        return getattr(sgd, name)
    if name in ("CrossEntropyLoss", "FocalLoss", "WeightCE", "OIMLoss", "oim", "accuracy", "cross_entropy_train"):
        from . import loss
        return getattr(loss, name)
    if name in ("DECFinedTrainer2Mixin", "DECJointTrainer2Mixin"):
        from . import trainers
        return getattr(trainers, name)
    if name in ("create", "names", "InceptionNet"):      # the model factory with all six names (reid/models/__init__.py)
        from . import inception
        return getattr(inception, name)
    if name in ("TestDataset", "TestBatchLoader", "FiveCrops", "parse_market_name", "ten_crop_batch", "crop_mean", "extract_feature_matrix",
                "multi_query_pool", "evaluate"):      # reid/extract_feature.py (its extract_features: ssg_amd.extract_feature.extract_features)
        from . import extract_feature
        return getattr(extract_feature, name)
    if name in ("ResNet", "synthetic_state_dict"):
        from . import resnet
        return getattr(resnet, name)
    raise AttributeError(name)
