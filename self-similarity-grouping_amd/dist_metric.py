"""DistanceMetric -- host-side mirror of reid/dist_metric.py:9-29: the object the drivers build from `--dist-metric` and hand to
`Evaluator.evaluate(..., metric=)`.

`train` keeps the embeddings on the device from the extraction to the fit (the reference collects a dictionary of CPU tensors and
stacks `features.values()`, which Python 3 refuses).  One GPU: the fit is not sharded."""
import numpy as np

from .metric_learning import get_metric


class DistanceMetric(object):
    def __init__(self, algorithm='euclidean', *args, **kwargs):
        super(DistanceMetric, self).__init__()
        self.algorithm = algorithm
        self.metric = get_metric(algorithm, *args, **kwargs)

    def train(self, model, data_loader, rng=np.random):
        """dist_metric.py:15-20.  rng: the numpy stream KISSME.fit draws its non-matching pairs from (the reference's is np.random)"""
        if self.algorithm == 'euclidean':
            return
        from .evaluators import extract_embeddings
        features, _, labels = extract_embeddings(model, data_loader, for_eval=True)     # extract_features' default (evaluators.py:18)
        labels = np.asarray([float(pid) for pid in labels], dtype=np.float32)          # torch.Tensor(list(labels.values())).numpy()
        if self.algorithm == 'kissme':
            self.metric.fit(features, labels, rng=rng)
        else:
            self.metric.fit(features, labels)

    def transform(self, X):
        """dist_metric.py:22-29: tensors come back as tensors (on their own device), arrays as arrays"""
        return self.metric.transform(X)
