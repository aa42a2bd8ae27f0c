"""Host-side mirror of the grouping helper of semitraining.py (SSG++) that differs from selftraining.py's.

semitraining.py:324-360 `generate_selflabel` is selftraining.py:280-313's with one change: the eps rule runs (and the DBSCAN
estimators are created and cached) at `n_iter == args.start_epoch` instead of at iteration 0, so that a resumed run
(`--start_epoch`) starts by clustering.  compute_dist and generate_dataloader are the same as selftraining.py's
(ssg_amd.selftraining.compute_dist / generate_dataset).
"""
from .cluster import DBSCAN, eps_rule_dbscan


def generate_selflabel(e_dist, r_dist, n_iter, args, cluster_list=[]):   # noqa: B006 (mutable default kept: reference :324)
    """semitraining.py:324-360.  `args` needs `.no_rerank`, `.rho` and `.start_epoch`."""
    labels_list = []
    for s in range(len(r_dist)):
        tmp_dist = e_dist[s] if args.no_rerank else r_dist[s]
        if n_iter == args.start_epoch:
            # the eps rule and the first fit as one device chain (see selftraining.generate_selflabel)
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
