"""SSG++ label estimation and selection on the device -- host-side mirror of reid/eug.py (caller: semitraining.py:228-244).

Device-level API:
  estimate_label_device(u_feas, l_feas, l_label, rerank=True, ...)  eug.py:193-251 on device or numpy features
  dissimilarity_from_dist(re_rank_dist, l_label)                     the loop of eug.py:232-240 on a [Nu, Nl] matrix
  nearest_labelled(u_feas, l_feas, l_label)                           the loop of eug.py:205-214 (rerank=False), bit for bit
  select_top(scores, k, labels=None)                                   select_top_data / select_top_true_data (eug.py:277-289)
and the drop-in `EUGMixin` for the reference's EUG class (INTEGRATION.md "SSG++"):

    from reid.eug import *
    from ssg_amd.eug import EUGMixin
    class EUG(EUGMixin, EUG): pass

plus `updata_lable`, the one-shot split of eug.py:325-385 (host only, the same split for the same seed).
Results keep the reference's types: float64 numpy arrays of labels, scores and confidences, a bool mask.
"""
import os.path as osp
import pickle
import random

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream

CLASSIFICATION_UNSUPPORTED = ("EUG 'Classification' mode is not supported: it needs num_classes > 0, and semitraining.py:121 builds the "
                              "model with num_class = 0, so the reference fails its own assert in get_Classification_result")


def _device(device=None):
    return torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)


def _dev(x, dtype, device):
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x))
    return torch.as_tensor(x).to(device=device, dtype=dtype).contiguous()


def _host(t):
    return t.cpu().numpy()


def nearest_labelled(u_feas, l_feas, l_label, device=None):
    """rerank=False (eug.py:205-214): for every u row, argmin_j np.linalg.norm(l_feas - u, axis=1)[j] bit for bit.
    Returns device tensors (labels int64 = l_label[argmin], scores float64 = -min, argmin int32, min float32)."""
    L = _lib.lib()
    dev = _device(device)
    u = _dev(u_feas, torch.float32, dev); l = _dev(l_feas, torch.float32, dev)
    lab = _dev(np.asarray(l_label).astype(np.int64), torch.int64, dev)
    if u.dim() != 2 or l.dim() != 2 or u.shape[1] != l.shape[1] or lab.numel() != l.shape[0]:
        raise ValueError("nearest_labelled: u [Nu,d], l [Nl,d] and l_label [Nl] expected, got %s %s %s" % (tuple(u.shape), tuple(l.shape), tuple(lab.shape)))
    nu, d = u.shape
    nl = l.shape[0]
    ns = int(L.ssg_eug_nn_splits(nu, nl))
    part_val = torch.empty(ns * nu, dtype=torch.float32, device=dev); part_idx = torch.empty(ns * nu, dtype=torch.int32, device=dev)
    argmin = torch.empty(nu, dtype=torch.int32, device=dev); minval = torch.empty(nu, dtype=torch.float32, device=dev)
    labels = torch.empty(nu, dtype=torch.int64, device=dev); scores = torch.empty(nu, dtype=torch.float64, device=dev)
    check(L.ssg_eug_nn_f32(ptr(u), nu, ptr(l), nl, d, ptr(lab), ns, ptr(part_val), ptr(part_idx), ptr(argmin), ptr(minval), ptr(labels),
                           ptr(scores), stream()), "ssg_eug_nn_f32")
    return labels, scores, argmin, minval


def dissimilarity_from_dist(re_rank_dist, l_label, device=None, return_argmin=False):
    """The loop of eug.py:232-240 on a [Nu, Nl] float32 matrix (device tensor or numpy): labels = l_label[argmin] (float64),
    scores = -min (float64), confidence = 1 - min / np.max(column argmin) (float32 arithmetic, float64 array), bit for bit."""
    L = _lib.lib()
    dev = _device(device)
    D = _dev(re_rank_dist, torch.float32, dev)
    lab = _dev(np.asarray(l_label).astype(np.int64), torch.int64, dev)
    nu, nl = D.shape
    if lab.numel() != nl:
        raise ValueError("dissimilarity_from_dist: l_label has %d entries for %d columns" % (lab.numel(), nl))
    ws = torch.empty(65 * nl, dtype=torch.float32, device=dev)
    argmin = torch.empty(nu, dtype=torch.int32, device=dev)
    labels = torch.empty(nu, dtype=torch.int64, device=dev)
    scores = torch.empty(nu, dtype=torch.float64, device=dev); conf = torch.empty(nu, dtype=torch.float64, device=dev)
    check(L.ssg_eug_dist_label_f32(ptr(D), nu, nl, ptr(lab), ptr(ws), ptr(argmin), ptr(labels), ptr(scores), ptr(conf), stream()),
          "ssg_eug_dist_label_f32")
    out = (_host(labels).astype(np.float64), _host(scores), _host(conf))
    return out + (_host(argmin),) if return_argmin else out


def estimate_label_device(u_feas, l_feas, l_label, rerank=True, k1=20, k2=6, lambda_value=0.3, weight=False, device=None):
    """get_Dissimilarity_result (eug.py:193-251) without the feature extraction: u_feas [Nu,d], l_feas [Nl,d] (device tensors or
    numpy, L2-normalised embeddings).  rerank=True: re_ranking_init(u, l) on the device (the [Nu,Nl] matrix never leaves it), then
    dissimilarity_from_dist; returns (labels, scores, confidence) if weight else (labels, scores).  rerank=False: nearest_labelled
    (the reference returns two arrays there whatever `weight` says, and so does this).  float64 numpy arrays."""
    dev = _device(device)
    if not rerank:
        labels, scores, _, _ = nearest_labelled(u_feas, l_feas, l_label, device=dev)
        return _host(labels).astype(np.float64), _host(scores)
    from .rerank import re_ranking_init_device
    D = re_ranking_init_device(u_feas, l_feas, k1=k1, k2=k2, lambda_value=lambda_value, device=dev)
    labels, scores, conf = dissimilarity_from_dist(D, l_label, device=dev)
    return (labels, scores, conf) if weight else (labels, scores)


def select_top(scores, k, labels=None, device=None):
    """Bool mask of the k largest scores (eug.py:284-289 select_top_data); with labels, entries labelled -1 are dropped from the
    selection (eug.py:277-282 select_top_true_data).  np.argsort(-scores) order: NaN last.  Equal scores that straddle the cut
    are taken lowest index first; numpy's own choice among them depends on the host CPU's sort."""
    L = _lib.lib()
    dev = _device(device)
    s = _dev(np.asarray(scores) if not torch.is_tensor(scores) else scores, torch.float64, dev).reshape(-1)
    n = s.numel()
    k = int(k)
    if n == 0:
        return np.zeros(0, dtype=bool)
    if not 0 <= k <= n:
        raise ValueError("select_top: k = %d outside [0, %d]" % (k, n))
    lab = None
    if labels is not None:
        lab = _dev(np.asarray(labels) if not torch.is_tensor(labels) else labels, torch.float64, dev).reshape(-1)
        if lab.numel() != n:
            raise ValueError("select_top: %d labels for %d scores" % (lab.numel(), n))
    mask = torch.empty(n, dtype=torch.uint8, device=dev)
    check(L.ssg_eug_select_top(ptr(s), n, k, ptr(lab), ptr(mask), stream()), "ssg_eug_select_top")
    return _host(mask).astype(bool)


class EUGMixin(object):
    """Overrides of reid/eug.py's EUG for the label step of SSG++ (class EUG(EUGMixin, EUG): pass).  The host object keeps the
    reference's attributes (model, u_data, l_data, u_label, l_label, mode, rerank, get_dataloader); features are extracted with
    ssg_amd.extract_embeddings and stay on the device."""

    def get_feature(self, dataset):
        from .evaluators import extract_embeddings
        loader = self.get_dataloader(dataset, training=False)
        feats, _, _ = extract_embeddings(self.model, loader, for_eval=True)
        return feats

    def get_Classification_result(self):
        raise NotImplementedError(CLASSIFICATION_UNSUPPORTED)

    def get_Dissimilarity_result(self, weight=False):
        u_feas = self.get_feature(self.u_data)
        l_feas = self.get_feature(self.l_data)
        print("u_features", tuple(u_feas.shape), "l_features", tuple(l_feas.shape))
        out = estimate_label_device(u_feas, l_feas, self.l_label, rerank=self.rerank, weight=weight)
        labels = out[0]
        n = len(labels)
        num_correct_pred = int((np.asarray(self.u_label) == labels.astype(np.int64)).sum())
        print("{} predictions on all the unlabeled data: {} of {} is correct, accuracy = {:0.3f}".format(
            self.mode, num_correct_pred, n, num_correct_pred / n))
        return out

    def estimate_label(self):
        print("label estimation by {} mode.".format(self.mode))
        if self.mode == "Dissimilarity":
            pred_label, pred_score = self.get_Dissimilarity_result()[:2]
            return pred_label, pred_score
        if self.mode == "Classification":
            raise NotImplementedError(CLASSIFICATION_UNSUPPORTED)
        if self.mode == "Weight":
            if not self.rerank:
                raise ValueError("EUG 'Weight' mode needs rerank=True: the reference's rerank=False branch returns no confidence")
            return self.get_Dissimilarity_result(True)
        raise ValueError(self.mode)

    def select_top_true_data(self, pred_label, pred_score, nums_to_select):
        return select_top(pred_score, nums_to_select, labels=pred_label)

    def select_top_data(self, pred_score, nums_to_select):
        return select_top(pred_score, nums_to_select)

    def generate_new_train_data(self, sel_idx, pred_y):
        return generate_new_train_data(self.l_data, self.u_data, self.u_label, sel_idx, pred_y)


class EUGTrainLoaderMixin(object):
    """Opt-in override of reid/eug.py:62-96 get_dataloader (class EUG(EUGTrainLoaderMixin, EUGMixin, EUG): pass): the training loader of
    the num_classes == 0 branch -- RandomSizedRectCrop, RandomHorizontalFlip, ToTensor, Normalize, RandomErasing(0.5, sh=0.2, r1=0.3) with
    RandomIdentitySampler(dataset, num_instances), drop_last -- is an ssg_amd.trainloader.GpuTrainLoader with the same random streams;
    every other loader is the base class's."""

    def get_dataloader(self, dataset, training=False):
        if not (training and self.num_classes == 0):
            return super(EUGTrainLoaderMixin, self).get_dataloader(dataset, training=training)
        from .trainloader import GpuTrainLoader, TrainTransform
        tf = TrainTransform(self.data_height, self.data_width, crop="random_rect", flip_p=0.5, mean=(0.485, 0.456, 0.406),
                            std=(0.229, 0.224, 0.225), erase_p=0.5, sh=0.2, r1=0.3)
        print("create dataloader for Training with batch_size {}".format(self.batch_size))
        return GpuTrainLoader(dataset, root=None, transform=tf, batch_size=self.batch_size, num_instances=self.num_instances,
                              num_workers=self.data_workers)


def generate_new_train_data(l_data, u_data, u_label, sel_idx, pred_y):
    """eug.py:292-310: the labelled list followed by [fname, int(predicted label), camid] of every selected unlabelled image."""
    selected = []
    correct = 0
    for i in np.nonzero(np.asarray(sel_idx))[0]:
        y = int(pred_y[i])
        selected.append([u_data[i][0], y, u_data[i][2]])
        correct += int(u_label[i] == y)
    total = len(selected)
    acc = correct / total              # (no selection: ZeroDivisionError, like the reference)
    new_train_data = l_data + selected
    print("selected pseudo-labeled data: {} of {} is correct, accuracy: {:0.4f}  new train data: {}".format(
        correct, total, acc, len(new_train_data)))
    return new_train_data


def updata_lable(dataset, label, name, sample='random', load_path='random_split/', seed=0):
    """eug.py:325-385: the one-shot split of the target set, (unlabelled, labelled) lists of [path, pid, camid].  Reseeds numpy and
    `random` with `seed` and consumes numpy's global generator in the reference's order, so the same seed gives the same split;
    the split is cached in `load_path + sample + '_' + name + '.pkl'` and read back from there when it exists.
    sample='random': the first len(set(label)) - 1 images of the shuffled trainval list are labelled; sample='cluster': one
    shuffled-first member of every cluster (label != -1, clusters in order of first appearance)."""
    np.random.seed(seed)
    random.seed(seed)
    path = load_path + sample + '_' + name + '.pkl'
    if osp.exists(path):
        with open(path, "rb") as fp:
            split = pickle.load(fp)
        label_dataset, unlabel_dataset = split["label set"], split["unlabel set"]
        print("  labeled  |   N/A | {:8d}".format(len(label_dataset)))
        print("  unlabel  |   N/A | {:8d}".format(len(unlabel_dataset)))
        print("\nLoad one-shot split from", path)
        return unlabel_dataset, label_dataset
    print("Randomly Create new one-shot split and save it to", path)
    items = [[osp.join(dataset.images_dir, f), pid, camid] for f, pid, camid in dataset.trainval]
    if sample == 'random':
        label_dataset = list(items)
        np.random.shuffle(label_dataset)
        label_dataset = label_dataset[:len(set(label)) - 1]
    elif sample == 'cluster':
        groups = {}
        for i, it in enumerate(items):
            if label[i] != -1:
                groups.setdefault(label[i], []).append(list(it))
        label_dataset = []
        for members in groups.values():
            np.random.shuffle(members)
            label_dataset.append(members[0])
    else:
        raise ValueError("updata_lable: sample must be 'random' or 'cluster', got %r" % (sample,))
    chosen = set(f for f, _, _ in label_dataset)
    unlabel_dataset = [list(it) for it in items if it[0] not in chosen]
    print("  labeled    | N/A | {:8d}".format(len(label_dataset)))
    print("  unlabeled  | N/A | {:8d}".format(len(unlabel_dataset)))
    with open(path, "wb") as fp:
        pickle.dump({"label set": label_dataset, "unlabel set": unlabel_dataset}, fp)
    return unlabel_dataset, label_dataset
