"""Trainer overrides for the fine-tune phase with the DEC head (--dce-loss): `_forward` of reid/trainers.py's FinedTrainer2 (:254-282)
and JointTrainer2 (:440-495) with the DEC term -- target_distribution + nn.KLDivLoss(size_average=False) / B, a chain of about twenty
torch launches over float32 temporaries -- computed by `ssg_amd.dce.kl_loss` (two HIP launches, float64 sums).  Used like EUGMixin:

    from reid.trainers import FinedTrainer2, JointTrainer2
    class FinedTrainer2(DECFinedTrainer2Mixin, FinedTrainer2): pass
    class JointTrainer2(DECJointTrainer2Mixin, JointTrainer2): pass

Everything else is the reference's: which criterion sees which output, the list branches, the weight 3 on the DEC term of
FinedTrainer2's tensor branch (1 everywhere else), JointTrainer2 deciding on len(outputs) for both of its forwards, and the
precision that is returned."""
from . import dce


def _main_terms(criterions, outputs, pids, epoch):
    """global loss on outputs[1] + triplet loss on outputs[0] (every split against its own labels when it is a list) -> (loss, prec)"""
    loss, prec = criterions[1](outputs[1], pids[0], epoch)
    if isinstance(outputs[0], list):
        for i, part in enumerate(outputs[0]):
            loss = loss + criterions[0](part, pids[i], epoch)[0]
    else:
        loss = loss + criterions[0](outputs[0], pids[0], epoch)[0]
    return loss, prec


def _add_dec(loss, x3, tensor_weight):
    """loss + the DEC term of one forward, added in the reference's order: a list of assignments one by one with weight 1, a single
    one with `tensor_weight`"""
    if isinstance(x3, list):
        for q in x3:
            loss = loss + dce.kl_loss(q)
        return loss
    term = dce.kl_loss(x3)
    return loss + (term if tensor_weight == 1 else tensor_weight * term)


class DECFinedTrainer2Mixin(object):
    def _forward(self, inputs, pids, epoch):
        outputs = self.model(*inputs)
        loss, prec = _main_terms(self.criterions, outputs, pids, epoch)
        if len(outputs) == 3:
            loss = _add_dec(loss, outputs[2], 3)
        return loss, prec


class DECJointTrainer2Mixin(object):
    def _forward(self, inputs, pids, inputs_eug, pids_eug, epoch, w_eug=None):
        outputs = self.model(*inputs)
        loss_uns, prec = _main_terms(self.criterions, outputs, pids, epoch)
        if len(outputs) == 3:
            loss_uns = _add_dec(loss_uns, outputs[2], 1)
        outputs_eug = self.model(*inputs_eug)
        loss_os, prec_eug = self.criterions[1](outputs_eug[1], pids_eug, epoch)
        prec = prec + prec_eug
        if isinstance(outputs_eug[0], list):          # one-shot batch: every split against the same labels
            for part in outputs_eug[0]:
                loss_os = loss_os + self.criterions[0](part, pids_eug, epoch)[0]
        else:
            loss_os = loss_os + self.criterions[0](outputs_eug[0], pids_eug, epoch)[0]
        if len(outputs) == 3:                         # the reference tests `outputs` here too, not `outputs_eug`
            loss_os = _add_dec(loss_os, outputs_eug[2], 1)
        return loss_os + loss_uns, prec
