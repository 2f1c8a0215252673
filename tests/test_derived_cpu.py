"""acr_wsss_amd._derived on the CPU: the stamp of a weight, the per-owner store, the parameter stamp of the captured graphs and
the lookup that serves both graph caches -- none of it needs a GPU or the library."""
import warnings
from collections import OrderedDict

import pytest
import torch

from acr_wsss_amd import _derived as D


@pytest.fixture
def lin():
    torch.manual_seed(0)
    return torch.nn.Linear(8, 12)


def test_stored_form_is_served_until_the_stamp_moves(lin):
    wt = lin.weight.detach().t().contiguous()
    assert D.get(lin, "t", lin.weight) is None
    D.put(lin, "t", lin.weight, wt)
    assert D.get(lin, "t", lin.weight) is wt and D.get(lin, "img", lin.weight) is None
    with torch.no_grad():
        lin.weight.mul_(2.0)                                   # in-place through the parameter: the version moves
    assert D.get(lin, "t", lin.weight) is None
    D.put(lin, "t", lin.weight, wt)
    assert D.get(lin, "t", lin.weight) is wt
    lin.weight.data = lin.weight.data.clone()                  # a re-allocated storage: the address moves
    assert D.get(lin, "t", lin.weight) is None
    D.put(lin, "t", lin.weight, wt)
    lin.double()                                               # another dtype
    assert D.get(lin, "t", lin.weight) is None


def test_write_through_data_is_the_blind_spot_and_invalidate_the_remedy(lin):
    wt = lin.weight.detach().t().contiguous()
    D.put(lin, "t", lin.weight, wt)
    lin.weight.data.mul_(2.0)                                  # no version bump, same storage: NOT seen (documented in _derived.py)
    assert D.get(lin, "t", lin.weight) is wt and not torch.equal(wt, lin.weight.detach().t())
    D.invalidate(lin)
    assert D.get(lin, "t", lin.weight) is None and not D.entries(lin)


def test_entry_is_not_served_for_another_tensor(lin):
    D.put(lin, "img", lin.weight, torch.zeros(3))
    other = torch.nn.Linear(8, 12)
    assert D.get(lin, "img", other.weight) is None             # another tensor asked about on this owner
    assert D.get(other, "img", lin.weight) is None             # another owner holds nothing
    assert D.get(None, "img", lin.weight) is None
    D.put(other, "img", lin.weight, torch.ones(3))             # stored on an owner whose parameter is another tensor
    assert D.get(other, "img", lin.weight) is None


def test_invalidate_on_a_parent_clears_every_form_on_every_child():
    model = torch.nn.Sequential(torch.nn.Linear(8, 12), torch.nn.Sequential(torch.nn.Linear(12, 8), torch.nn.ReLU()))
    lins = [m for m in model.modules() if isinstance(m, torch.nn.Linear)]
    for m in lins:
        for form in ("t", "img", "img_t"):
            D.put(m, form, m.weight, torch.zeros(1))
    D.entries(model, create=True)["linears"] = lins
    assert len(D.held(model.modules())) == 4 and len(D.held(lins[:1])) == 2
    D.invalidate(model, D.IMAGES)                              # some forms only
    assert not D.held(model.modules()) and all(D.get(m, "t", m.weight) is not None for m in lins) and D.entries(model)
    D.invalidate(model)
    assert not any(D.entries(m) for m in model.modules())


def test_parameter_stamp():
    model = torch.nn.Sequential(torch.nn.Linear(8, 12), torch.nn.LayerNorm(12), torch.nn.Linear(12, 4))
    s0 = D.weights_stamp(model)
    assert s0 == D.weights_stamp(model) and not D.weights_moved(s0, model)
    for p in model.parameters():                               # an in-place update of any ONE parameter
        s = D.weights_stamp(model)
        with torch.no_grad():
            p.add_(1.0)
        assert D.weights_stamp(model) != s and D.weights_moved(s, model)
    s1 = D.weights_stamp(model)
    model[1].bias.data = model[1].bias.data.clone()            # a re-allocated storage
    assert D.weights_stamp(model) != s1 and D.weights_moved(s1, model)


def test_stem_generation_is_part_of_the_stamp():
    class Stem:
        frozen_generation, refreshed = 3, 0

        def refresh_frozen(self, dtype):
            self.refreshed += 1

    model, stem = torch.nn.Linear(4, 4), Stem()
    s = D.weights_stamp(model, stem)
    assert not D.weights_moved(s, model, stem, torch.float32) and stem.refreshed == 1      # brought up to date, then compared
    stem.frozen_generation += 1
    assert D.weights_moved(s, model, stem, torch.float32)
    with torch.no_grad():
        model.weight.add_(1.0)
    n = stem.refreshed
    assert D.weights_moved(s, model, stem, torch.float32) and stem.refreshed == n          # parameters moved: the stem is not touched


class Holder:
    pass


class FakeGraph:
    def __init__(self):
        self.ok = True

    def valid(self):
        return self.ok


class Builder:
    def __init__(self, fail=False):
        self.calls, self.fail = 0, fail

    def __call__(self):
        self.calls += 1
        if self.fail:
            raise RuntimeError("cannot capture\nsecond line")
        return FakeGraph()


def lookup(holder, key, build, sightings=2, bound=8):
    return D.graph_lookup(holder, "_pass_graphs", key, sightings, bound, lambda g: g.valid(), build, lambda e: "capture failed (%s)" % str(e).splitlines()[0])


def test_graph_lookup_sightings_hits_and_staleness():
    h, build = Holder(), Builder()
    assert lookup(h, "a", build) is None and build.calls == 0              # first sighting: eager, nothing built
    g = lookup(h, "a", build)
    assert isinstance(g, FakeGraph) and build.calls == 1                   # second sighting builds
    assert type(h._pass_graphs) is OrderedDict and type(h._graph_sightings) is OrderedDict
    assert lookup(h, "b", build) is None and isinstance(lookup(h, "b", build), FakeGraph) and build.calls == 2
    assert list(h._pass_graphs) == ["a", "b"]
    assert lookup(h, "a", build) is g and build.calls == 2                 # a hit: the same object, now most recent
    assert list(h._pass_graphs) == ["b", "a"]
    g.ok = False
    g2 = lookup(h, "a", build)                                             # stale: rebuilt on this very call
    assert isinstance(g2, FakeGraph) and g2 is not g and build.calls == 3 and h._pass_graphs["a"] is g2
    one = Builder()
    assert isinstance(lookup(h, "c", one, sightings=1), FakeGraph) and one.calls == 1      # sightings = 1: the first call builds


def test_graph_lookup_caches_a_failed_capture():
    h, build = Holder(), Builder(fail=True)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        assert lookup(h, "a", build, sightings=1) is None
        assert lookup(h, "a", build, sightings=1) is None
        assert lookup(h, "a", build, sightings=1) is None
    assert build.calls == 1 and h._pass_graphs["a"] is False
    assert [str(x.message) for x in w] == ["capture failed (cannot capture)"]


def test_graph_lookup_bound_evicts_the_least_recently_used():
    h, build = Holder(), Builder()
    a = lookup(h, "a", build, sightings=1, bound=2)
    lookup(h, "b", build, sightings=1, bound=2)
    assert lookup(h, "a", build, sightings=1, bound=2) is a                # "b" is now the least recently used
    lookup(h, "c", build, sightings=1, bound=2)
    assert list(h._pass_graphs) == ["a", "c"] and build.calls == 3
    D.drop_graphs([torch.nn.Identity()])                                     # nothing held: nothing to drop
    m = torch.nn.Sequential(torch.nn.Identity())
    m[0].__dict__.update(_pass_graphs=OrderedDict(), _prefix_graphs=OrderedDict(), _graph_sightings=OrderedDict())
    D.drop_graphs(m.modules())
    assert set(m[0].__dict__) >= {"_graph_sightings"} and "_pass_graphs" not in m[0].__dict__ and "_prefix_graphs" not in m[0].__dict__
    D.drop_graphs(m.modules(), sightings=True)
    assert "_graph_sightings" not in m[0].__dict__
