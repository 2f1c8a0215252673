"""Tensors derived from a weight, and when they are stale ("Derived weights").  Host code only: torch, no library.

A derived tensor is kept on the module that owns the weight, in ONE attribute {form: entry}, with a stamp of that weight.  Forms:
"t" (W^T, ops.WeightTransposes), "img" / "img_t" (split-product images of W / W^T, ops.weight_image), "frozen" (on the stem:
ResNetV2._standardised), "linears" / "wt_f32" (on a model: train.refresh_weight_transposes).

THE RULE: an entry is current iff its stamp -- autograd version, storage address, device, dtype, shape -- equals the weight's
now and the owner's parameter is the tensor asked about.  In-place updates through the parameter (an optimizer step,
load_state_dict), a re-allocated storage (``p.data = ...``), ``.to(device)`` and ``.float()`` all move the stamp.  THE BLIND
SPOT: a write through ``.data`` (``p.data.mul_()``, ``p.data.copy_()``, an EMA swap) moves nothing a stamp records.  THE REMEDY
after such a write: ``ACR.invalidate_caches()`` = ``invalidate`` + ``drop_graphs`` (captured graphs are stamped likewise)."""
from collections import OrderedDict

import torch

STORE = "_acr_derived"
IMAGES = ("img", "img_t")


def stamp(w):
    return (w._version, w.data_ptr(), w.device, w.dtype, w.shape)


def entries(owner, create=False):
    return owner.__dict__.setdefault(STORE, {}) if create else owner.__dict__.get(STORE, {})


def built_here(device):
    """(current stream, event behind what is queued on it): what an entry read across streams (CAM scales) remembers of its build."""
    cur = torch.cuda.current_stream(device)
    ev = torch.cuda.Event()
    ev.record(cur)
    return cur, ev


def put(owner, form, weight, tensor, built=(None, None)):
    """Keep ``tensor`` as ``form`` of ``owner``'s ``weight`` (never while capturing); without ``built``: for same-stream readers."""
    entries(owner, True)[form] = (stamp(weight), tensor) + built


def get(owner, form, weight):
    """The tensor kept as ``form`` if it is current for ``weight``, else None; ``owner`` (None: nothing is kept) owns a parameter
    named ``weight``.  A hit on another stream waits for the build."""
    e = entries(owner).get(form) if owner is not None else None
    if e is None or e[0] != stamp(weight) or owner._parameters["weight"].data_ptr() != e[0][1]:
        return None
    if e[2] is not None:
        cur = torch.cuda.current_stream(weight.device)
        if e[2] != cur and not torch.cuda.is_current_stream_capturing():
            cur.wait_event(e[3])
    return e[1]


def invalidate(tree, forms=None):
    """Drop every derived entry (or only ``forms``) of every module under ``tree``."""
    for m in tree.modules():
        for f in (forms or list(entries(m))):
            entries(m).pop(f, None)


def held(modules):
    """The image tensors stored for ``modules`` right now (a captured graph pins the ones its launches read)."""
    return [e[1] for m in modules for f, e in entries(m).items() if f in IMAGES]


def weights_stamp(module, stem=None):
    """What a graph captured over ``module`` read: parameter addresses and versions, the generation of the stem's frozen cache."""
    return tuple((p.data_ptr(), p._version) for p in module.parameters()), (stem.frozen_generation if stem is not None else 0)


def weights_moved(stamped, module, stem=None, dtype=None):
    """Have the parameters or the stem cache moved since ``stamped``?"""
    if stamped[0] != weights_stamp(module)[0]:
        return True
    if stem is not None:
        stem.refresh_frozen(dtype)       # rebuilds the cache when a conv weight changed in place; then the generation moves
    return stem is not None and stem.frozen_generation != stamped[1]


def graph_lookup(holder, attr, key, sightings, bound, valid, build, failed):
    """The graph kept under ``key`` in the LRU ``holder.<attr>`` (at most ``bound`` entries), or None for eager launches.  A stale
    one is captured again at once; a new key the ``sightings``-th time it is asked for (a capture costs about four passes and a
    private pool; the count survives invalidation).  ``build()`` raising RuntimeError warns and caches False: the key stays eager."""
    cache = holder.__dict__.setdefault(attr, OrderedDict())
    g = cache.get(key)
    if g is not None and g is not False and not valid(g):
        del cache[key]
        g = None
    if g is None:
        seen = holder.__dict__.setdefault("_graph_sightings", OrderedDict())
        seen[attr, key] = n = seen.get((attr, key), 0) + 1
        seen.move_to_end((attr, key))
        while len(seen) > 64:
            seen.popitem(last=False)
        if n < sightings:
            return None
        try:
            g = build()
        except RuntimeError as e:
            import warnings
            warnings.warn(failed(e))                       # called while ``e`` is being handled: it may format the traceback
            if torch.cuda.is_initialized():
                torch.cuda.synchronize()
            g = False
        cache[key] = g
        while len(cache) > bound:
            cache.popitem(last=False)
    cache.move_to_end(key)
    return g or None


def drop_graphs(modules, sightings=False):
    """Drop the captured graphs ``modules`` hold (their private pools go back to the allocator)."""
    for m in modules:
        for attr in ("_prefix_graphs", "_pass_graphs") + (("_graph_sightings",) if sightings else ()):
            m.__dict__.pop(attr, None)
