"""What the train-mode layers (ssg_amd/batchnorm.py, conv.py, conv_strided.py, head.py) share: the GPU check, the bookkeeping that
sends a gradient back where its input lives, the ValueError idiom of the argument checks, and the walk that swaps torch modules of a
built model for their device counterparts."""
import torch

from ._lib import SSGError


def device(module):
    """the current GPU; `module` names the caller in the message (there is no CPU fallback)"""
    if not torch.cuda.is_available():
        raise SSGError("ssg_amd.%s needs a GPU (there is no CPU fallback)" % module)
    return torch.device("cuda", torch.cuda.current_device())


def src(*tensors):
    """(device, dtype) of every input of a forward, None for an input that is None: what `back` needs, kept in ctx"""
    return tuple(None if t is None else (t.device, t.dtype) for t in tensors)


def back(grad, where):
    """the gradient on the device and in the dtype of its input (`where`: that input's entry of `src`); None stays None"""
    return None if grad is None or where is None else grad.to(device=where[0], dtype=where[1])


def refuse(fn, why):
    """raise ValueError naming the function and the rule when `why` is a rule (not None)"""
    if why is not None:
        raise ValueError(fn + ": " + why)


def adopt(new, old, parameters=(), buffers=()):
    """`new` in place of `old`: it holds the same Parameter and buffer objects under these names and is in the same mode"""
    for name in parameters:
        new._parameters[name] = old._parameters[name]
    for name in buffers:
        new._buffers[name] = old._buffers[name]
    new.training = old.training
    return new


def swap_modules(model, attr, family, exact, on_device, swap, after=None):
    """Walk `model` depth-first in `_modules` order (through nn.DataParallel's `.module` like through any child) and replace modules
    of one family by their device counterparts:

        a child that is None or for which `on_device(child)` holds is left alone and not listed;
        an instance of `family` whose type is one of `exact` (torch's own classes, no subclass) becomes `swap(child)` unless that is
        None; every other instance of the family is listed by its qualified name;
        anything else is walked into, and `after(module)`, when given, is called on it once its children are done -- also on `model`.

    The list is stored as `model.<attr>`.  Returns the model."""
    skipped = []

    def walk(parent, prefix):
        for name, child in list(parent._modules.items()):
            if child is None or on_device(child):
                continue
            if isinstance(child, family):
                new = swap(child) if type(child) in exact else None
                if new is None:
                    skipped.append(prefix + name)
                else:
                    parent._modules[name] = new
                continue
            walk(child, prefix + name + ".")
        if after is not None:
            after(parent)

    walk(model, "")
    setattr(model, attr, skipped)
    return model
