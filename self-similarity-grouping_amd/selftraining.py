"""Host-side mirror of the grouping helpers of selftraining.py (reference :255-313).

`compute_dist` and `generate_selflabel` keep the reference's names, argument order and
return structure so that selftraining.py can import them instead of its own definitions
(INTEGRATION.md).  Differences, all deliberate and documented in DESIGN.md:
  * distances stay on the GPU as `DistHandle`s unless `materialize=True`;
  * with no_rerank=True the euclidean matrices are kept (the reference discards them at
    selftraining.py:260-266 and then crashes in generate_selflabel on `[]`);
  * the cached "cluster" objects are `ssg_amd.cluster.DBSCAN` instances (eps frozen after
    iteration 0 exactly like selftraining.py:283-298).
"""
import numpy as np
import torch

from .cluster import DBSCAN, AffinityPropagation, as_handle, eps_rule, eps_rule_dbscan  # noqa: F401
from .rerank import DeviceBackedArray, re_ranking_device


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


VARIANTS = ("kreciprocal", "plain", "hausdorff")


def compute_dist(source_features, target_features, lambda_value, no_rerank, num_split=2, materialize=False, group=None, grouping="auto",
                 variant="kreciprocal", k=20, memory_save=False):
    """selftraining.py:255-277.  Features: torch tensors (CPU or CUDA) or numpy arrays,
    a list of S+1 per-split tensors or a single tensor.  Returns (euclidean_dist_list,
    rerank_dist_list) with one entry per split.

    group (torch.distributed) + grouping: 'shard' = every rank computes its `shard_bounds` row block and the small tables are
    all-gathered; 'replicate' = every rank runs the whole problem on its own GPU with no collective at all (the features are
    replicated on every rank anyway) -- identical handles, identical labels on every rank; 'auto' (default) = `dist.choose_grouping`:
    the form its time model predicts to be faster for this N and world size (small problems replicate).

    variant: which of the reference's three re-rank distances -- 'kreciprocal' (reid/rerank.py, the default: today's path),
    'plain' (reid/rerank_plain.py) or 'hausdorff' (reid/rerank_hausdorff.py).  The last two run on one GPU only (group must be
    None); `k` and `memory_save` (the reference's k and MemorySave) reach these two only -- the default variant keeps its own k1 / k2;
    their handles go on to `generate_selflabel` like the default's.  With no_rerank=True no re-rank distance is computed, so the
    variant makes no difference: every variant returns the same euclidean handles."""
    if variant not in VARIANTS:
        raise ValueError("compute_dist: variant must be one of %r, got %r" % (VARIANTS, variant))
    if variant != "kreciprocal" and group is not None:
        raise ValueError("compute_dist: variant=%r runs on a single GPU (group must be None)" % (variant,))
    euclidean_dist_list, rerank_dist_list = [], []
    if not isinstance(source_features, list):
        source_features, target_features = [source_features], [target_features]
    dev = _dev()
    for s, t in zip(source_features, target_features):
        s = torch.as_tensor(s).to(dev, torch.float32); t = torch.as_tensor(t).to(dev, torch.float32)
        row0, nrows, grp = 0, None, None
        if group is not None:
            import torch.distributed as dist
            from .dist import choose_grouping, shard_bounds
            if choose_grouping(t.shape[0], dist.get_world_size(group), grouping) == "shard":
                row0, row1 = shard_bounds(t.shape[0], dist.get_rank(group), dist.get_world_size(group))   # ragged N allowed
                nrows, grp = row1 - row0, group
        if variant != "kreciprocal" and not no_rerank:
            if variant == "plain":
                from .rerank_plain import re_ranking_plain_device as other
            else:
                from .rerank_hausdorff import re_ranking_hausdorff_device as other
            h = other(s, t, k=k, lambda_value=lambda_value, memory_save=memory_save)
        else:
            h = re_ranking_device(s, t, lambda_value=lambda_value, no_rerank=no_rerank, keep_euclid=no_rerank, row0=row0, nrows=nrows, group=grp,
                                  validate=materialize)     # fused path: the status words are read by generate_selflabel's first round trip
        if materialize:
            from . import hostio
            if no_rerank:
                euclidean_dist_list.append(hostio.to_host(h.euclid).numpy()); rerank_dist_list.append(None)
            else:
                f = DeviceBackedArray.attach(hostio.final_dist_to_host(h).numpy(), h)
                euclidean_dist_list.append([]); rerank_dist_list.append(f)
        else:
            euclidean_dist_list.append(h if no_rerank else [])
            rerank_dist_list.append(None if no_rerank else h)
    return euclidean_dist_list, rerank_dist_list


def generate_selflabel(e_dist, r_dist, n_iter, args, cluster_list=[]):   # noqa: B006 (mutable default kept: reference :280)
    """selftraining.py:280-313: eps rule at iteration 0 (estimator cached, eps frozen), then
    `cluster.fit_predict` per split.  `args` needs `.no_rerank` and `.rho`."""
    labels_list = []
    for s in range(len(r_dist)):
        tmp_dist = e_dist[s] if args.no_rerank else r_dist[s]
        if n_iter == 0:
            # eps rule + first fit as ONE device chain with one read-back (cluster.eps_rule_dbscan: the same eps, labels and core samples
            # as eps_rule followed by DBSCAN.fit); the estimator is cached with its eps exactly like selftraining.py:283-298
            eps, _, _, labels, core = eps_rule_dbscan(tmp_dist, args.rho, min_samples=4)
            print('eps in cluster: {:.3f}'.format(eps))
            cluster = DBSCAN(eps=eps, min_samples=4, metric='precomputed', n_jobs=8)
            cluster.labels_, cluster.core_sample_indices_, cluster.n_features_in_ = labels, core, len(labels)
            cluster_list.append(cluster)
            print('Clustering and labeling...')
        else:
            cluster = cluster_list[s]
            print('Clustering and labeling...')
            labels = cluster.fit_predict(tmp_dist)
        num_ids = len(set(labels.tolist())) - 1
        print('Iteration {} have {} training ids'.format(n_iter + 1, num_ids))
        labels_list.append(labels)
    return labels_list, cluster_list


def _similarity(dist):
    """-1.0 * the distance as a float64 CUDA tensor the estimator may overwrite; a device handle is negated on the device"""
    from .rerank import DistHandle
    valid = getattr(dist, "valid_handle", None)
    h = dist if isinstance(dist, DistHandle) else (valid() if callable(valid) else None)
    if isinstance(h, DistHandle):
        if h.group is not None:
            raise ValueError("generate_selflabel_affinity runs on a single GPU: a row-sharded DistHandle is not supported")
        f = h.final_dist()
        return torch.neg(f) if h.mode == 2 else f.neg_()       # (mode 2: final_dist() is the handle's own matrix)
    return torch.neg(torch.as_tensor(np.asarray(dist) if not torch.is_tensor(dist) else dist).to(_dev(), torch.float64))


def generate_selflabel_affinity(e_dist, r_dist, n_iter, args, cluster_list=[]):   # noqa: B006 (mutable default kept: reference :280)
    """selftraining.py:280-313 with its commented lines switched on (:302 `rerank_dist = -1.0 * rerank_dist  #for similarity matrix`,
    :308 `num_ids = len(set(labels))  ##for affinity_propagation cluster`): affinity propagation on the negated distance instead of the
    eps rule + DBSCAN.  The estimator is created at iteration 0 and cached in `cluster_list`; `args` needs `.no_rerank` and may carry
    `.ap_damping` (0.5), `.ap_preference` (None: the median) and `.ap_seed` (0)."""
    labels_list = []
    for s in range(len(r_dist)):
        tmp_dist = e_dist[s] if args.no_rerank else r_dist[s]
        if n_iter == 0:
            cluster = AffinityPropagation(affinity='precomputed', copy=False, damping=getattr(args, "ap_damping", 0.5),
                                          preference=getattr(args, "ap_preference", None), random_state=getattr(args, "ap_seed", 0))
            cluster_list.append(cluster)
        else:
            cluster = cluster_list[s]
        print('Clustering and labeling...')
        labels = cluster.fit_predict(_similarity(tmp_dist))
        num_ids = len(set(labels.tolist()))
        print('Iteration {} have {} training ids'.format(n_iter + 1, num_ids))
        labels_list.append(labels)
    return labels_list, cluster_list


def generate_selflabel_optics(e_dist, r_dist, n_iter, args, cluster_list=[]):   # noqa: B006 (mutable default kept: reference :280)
    """selftraining.py:280-313 with OPTICS in the place of the eps rule + DBSCAN: a density clustering that does not stake the run on one
    eps.  The estimator is created at iteration 0 and cached in `cluster_list`; `args` needs `.no_rerank` and may carry `.optics_method`
    ('xi': labels with no eps at all; 'dbscan': the eps cut of the ordering), `.optics_xi` (0.05), `.optics_min_samples` (4) and
    `.optics_max_eps` (inf).  With 'dbscan', eps is the reference's rho rule (`cluster.eps_rule(dist, args.rho)`) at iteration 0, printed
    with the reference's line and frozen on the cached estimator like selftraining.py:283-298.  One GPU only."""
    from .optics import OPTICS
    labels_list = []
    for s in range(len(r_dist)):
        tmp_dist = e_dist[s] if args.no_rerank else r_dist[s]
        if n_iter == 0:
            method = getattr(args, "optics_method", "xi")
            eps = None
            if method == "dbscan":
                eps = float(eps_rule(tmp_dist, args.rho)[0])
                print('eps in cluster: {:.3f}'.format(eps))
            cluster = OPTICS(metric='precomputed', cluster_method=method, eps=eps, xi=getattr(args, "optics_xi", 0.05),
                             min_samples=getattr(args, "optics_min_samples", 4), max_eps=getattr(args, "optics_max_eps", np.inf))
            cluster_list.append(cluster)
        else:
            cluster = cluster_list[s]
        print('Clustering and labeling...')
        labels = cluster.fit_predict(tmp_dist)
        num_ids = len(set(labels[labels >= 0].tolist()))
        print('Iteration {} have {} training ids'.format(n_iter + 1, num_ids))
        labels_list.append(labels)
    return labels_list, cluster_list


def generate_selflabel_hdbscan(e_dist, r_dist, n_iter, args, cluster_list=[]):   # noqa: B006 (mutable default kept: reference :280)
    """selftraining.py:280-313 with HDBSCAN in the place of the eps rule + DBSCAN: labels with no eps, and a per-sample
    `probabilities_` on the cached estimator that a fine-tune phase can use as a weight.  The estimator is created at iteration 0 and
    cached in `cluster_list`; `args` needs `.no_rerank` and may carry `.hdbscan_min_cluster_size` (4, the reference's DBSCAN min_samples),
    `.hdbscan_min_samples` (None: min_cluster_size), `.hdbscan_method` ('eom'), `.hdbscan_epsilon` (0.0) and
    `.hdbscan_allow_single_cluster` (False).  One GPU only."""
    from .hdbscan import HDBSCAN
    labels_list = []
    for s in range(len(r_dist)):
        tmp_dist = e_dist[s] if args.no_rerank else r_dist[s]
        if n_iter == 0:
            cluster = HDBSCAN(metric='precomputed', min_cluster_size=getattr(args, "hdbscan_min_cluster_size", 4),
                              min_samples=getattr(args, "hdbscan_min_samples", None), cluster_selection_method=getattr(args, "hdbscan_method", "eom"),
                              cluster_selection_epsilon=getattr(args, "hdbscan_epsilon", 0.0),
                              allow_single_cluster=getattr(args, "hdbscan_allow_single_cluster", False))
            cluster_list.append(cluster)
        else:
            cluster = cluster_list[s]
        print('Clustering and labeling...')
        labels = cluster.fit_predict(tmp_dist)
        num_ids = len(set(labels[labels >= 0].tolist()))
        print('Iteration {} have {} training ids'.format(n_iter + 1, num_ids))
        labels_list.append(labels)
    return labels_list, cluster_list


def generate_selflabel_agglomerative(e_dist, r_dist, n_iter, args, cluster_list=[]):   # noqa: B006 (mutable default kept: reference :280)
    """selftraining.py:280-313 with bottom-up clustering in the place of DBSCAN: average or complete linkage cut at a distance gives
    compact clusters whose mean distance or diameter the cut bounds (the grouping of BUC and its successors).  The estimator is created
    at iteration 0 and cached in `cluster_list`; `args` needs `.no_rerank` and may carry `.agglo_linkage` ('average'), `.agglo_threshold`
    (None), `.agglo_n_clusters` (None) and `.agglo_min_cluster_size` (4, the reference's DBSCAN min_samples).  With neither a threshold
    nor a number of clusters the cut is the reference's rho rule (`cluster.eps_rule(dist, args.rho)`) at iteration 0, printed with the
    reference's line and frozen on the cached estimator like selftraining.py:283-298.  Clusters of fewer than `agglo_min_cluster_size`
    samples become -1 (generate_dataset drops them as it drops DBSCAN noise), the others are renumbered 0 .. k - 1 in order of first
    appearance.  One GPU only."""
    from .agglomerative import AgglomerativeClustering, _drop_small
    labels_list = []
    for s in range(len(r_dist)):
        tmp_dist = e_dist[s] if args.no_rerank else r_dist[s]
        if n_iter == 0:
            threshold, n_clusters = getattr(args, "agglo_threshold", None), getattr(args, "agglo_n_clusters", None)
            if threshold is None and n_clusters is None:
                threshold = float(eps_rule(tmp_dist, args.rho)[0])
                print('eps in cluster: {:.3f}'.format(threshold))
            cluster = AgglomerativeClustering(n_clusters=n_clusters, metric='precomputed', linkage=getattr(args, "agglo_linkage", "average"),
                                              distance_threshold=threshold)
            cluster_list.append(cluster)
        else:
            cluster = cluster_list[s]
        print('Clustering and labeling...')
        labels = _drop_small(cluster.fit_predict(tmp_dist), int(getattr(args, "agglo_min_cluster_size", 4)))
        num_ids = len(set(labels[labels >= 0].tolist()))
        print('Iteration {} have {} training ids'.format(n_iter + 1, num_ids))
        labels_list.append(labels)
    return labels_list, cluster_list


def generate_selflabel_sweep(e_dist, r_dist, n_iter, args, cluster_list=[]):   # noqa: B006 (mutable default kept: reference :280)
    """selftraining.py:280-313 with a silhouette-driven choice of eps in the place of the single frozen cut.  At iteration 0 the
    reference's rho rule gives eps0 (`cluster.eps_rule(dist, args.rho)`, printed with the reference's line) and an
    `OPTICS(metric='precomputed', cluster_method='dbscan', eps=eps0)` is cached in `cluster_list`.  Every iteration fits it once, takes
    the DBSCAN-like labels of the ordering at eps0 * f for every f of `.sweep_factors` ((0.6, 0.8, 1.0, 1.25, 1.5)) in O(N) each, scores
    all cuts in ONE pass over the matrix (`silhouette_many(dist, cuts, diagonal='zero', ignore_noise=True)`) and keeps the cut
    `silhouette.select_cut` chooses: the largest sum of the silhouettes of the clustered samples / N, noise counting as 0, the first
    maximum in list order, the factor 1.0 when no cut can be scored.  `args` needs `.no_rerank` and `.rho` and may carry
    `.sweep_factors` and `.sweep_min_samples` (4).  The estimator keeps `labels_` (the chosen cut), `sweep_factor_`, `sweep_eps_` and
    `sweep_scores_`.  The score is a heuristic whose effect on re-ID accuracy nobody has measured; the function is opt-in.  One GPU only."""
    from .optics import OPTICS, cluster_optics_dbscan
    from .silhouette import select_cut, silhouette_many
    labels_list = []
    for s in range(len(r_dist)):
        tmp_dist = e_dist[s] if args.no_rerank else r_dist[s]
        if n_iter == 0:
            eps0 = float(eps_rule(tmp_dist, args.rho)[0])
            print('eps in cluster: {:.3f}'.format(eps0))
            cluster = OPTICS(metric='precomputed', cluster_method='dbscan', eps=eps0, min_samples=getattr(args, "sweep_min_samples", 4))
            cluster_list.append(cluster)
        else:
            cluster = cluster_list[s]
        print('Clustering and labeling...')
        cluster.fit(tmp_dist)
        factors = [float(f) for f in getattr(args, "sweep_factors", (0.6, 0.8, 1.0, 1.25, 1.5))]
        cuts = [cluster_optics_dbscan(reachability=cluster.reachability_, core_distances=cluster.core_distances_, ordering=cluster.ordering_,
                                      eps=cluster.eps * f) for f in factors]
        best, scores = select_cut(factors, cuts, lambda valid: silhouette_many(tmp_dist, valid, diagonal='zero', ignore_noise=True))
        labels = cuts[best]
        cluster.labels_, cluster.sweep_factor_, cluster.sweep_eps_, cluster.sweep_scores_ = labels, factors[best], cluster.eps * factors[best], scores
        print('sweep factors {} scores {} -> factor {} (eps {:.3f})'.format(
            factors, ['skipped' if x is None else '{:.4f}'.format(x) for x in scores], factors[best], cluster.sweep_eps_))
        num_ids = len(set(labels[labels >= 0].tolist()))
        print('Iteration {} have {} training ids'.format(n_iter + 1, num_ids))
        labels_list.append(labels)
    return labels_list, cluster_list


def select_labeled(labels_list):
    """selftraining.py:315-324 join: keep sample i iff no split labelled it -1.
    Returns (kept indices, [per-split label lists])."""
    lab = np.stack([np.asarray(l) for l in labels_list], axis=1) if len(labels_list) else np.zeros((0, 0), np.int64)
    keep = np.nonzero((lab != -1).all(axis=1))[0]
    return keep, lab[keep]


def generate_dataset(trainval, labels_list, iter_n=None):
    """The dataset half of selftraining.py:315-324 generate_dataloader: [(fname, [label of split 0, ...], 0)] for every image of
    `trainval` ([(fname, pid, cam)], loader order) that no split labelled -1; prints the reference's progress line when
    iter_n is given.  (The DataLoader / RandomIdentitySampler the reference wraps around it belong to the fine-tune phase.)"""
    keep, lab = select_labeled(labels_list)
    new_dataset = [(trainval[int(i)][0], [lab[r, s] for s in range(lab.shape[1])], 0) for r, i in enumerate(keep)]
    if iter_n is not None:
        print('Iteration {} have {} training images'.format(iter_n + 1, len(new_dataset)))
    return new_dataset
