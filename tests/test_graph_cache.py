"""sgp_amd.nn.layers.graph_cache.GraphCache: hits, misses and eviction (no GPU)."""
import gc
import weakref

import torch

from sgp_amd.nn.layers.graph_cache import GraphCache


class Builder:
    """Counts its calls; every value is a new object."""

    def __init__(self):
        self.calls = 0

    def __call__(self):
        self.calls += 1
        return object()


def edges():
    return torch.tensor([[0, 1, 2], [1, 2, 0]])


def test_hits_and_misses():
    c, build = GraphCache(), Builder()
    ei, extra = edges(), (3, "cpu")
    a = c.get((ei, None), extra, build)                                # None among the tensors is accepted
    assert c.get((ei, None), extra, build) is a and build.calls == 1   # the same object and version: the same value
    ei[0, 0] = 2                                                       # an in-place write rebuilds
    b = c.get((ei, None), extra, build)
    assert b is not a and build.calls == 2
    assert c.get((ei, None), extra, build) is b and build.calls == 2
    other = ei.clone()                                                 # equal values, another tensor: another entry
    assert torch.equal(other, ei)
    d = c.get((other, None), extra, build)
    assert d is not b and build.calls == 3
    assert c.get((ei, None), extra, build) is b and c.get((other, None), extra, build) is d and build.calls == 3
    assert c.get((ei, None), (4, "cpu"), build) is not b and build.calls == 4      # extra is part of the key


def test_weights_are_part_of_the_key_and_of_the_version():
    c, build = GraphCache(), Builder()
    ei, w = edges(), torch.ones(3)
    a = c.get((ei, w), (3, "cpu"), build)
    assert c.get((ei, None), (3, "cpu"), build) is not a and build.calls == 2
    assert c.get((ei, w), (3, "cpu"), build) is a
    w.mul_(2.)
    assert c.get((ei, w), (3, "cpu"), build) is not a and build.calls == 3


def test_a_third_key_evicts_the_first_inserted():
    c, build = GraphCache(size=2), Builder()
    e1, e2, e3 = edges(), edges(), edges()
    a = c.get((e1,), 3, build)
    b = c.get((e2,), 3, build)
    assert c.get((e1,), 3, build) is a                                 # a hit does not renew: eviction is by insertion
    c.get((e3,), 3, build)
    assert build.calls == 3
    assert c.get((e2,), 3, build) is b and build.calls == 3            # the second inserted stayed
    assert c.get((e1,), 3, build) is not a and build.calls == 4        # the first inserted went


def test_a_stale_rebuild_leaves_the_other_graph_cached():
    """The rebuild of A after an in-place write, while the cache is full, replaces A's entry where it stands and evicts
    nothing: B's plan stays.  (The plan caches before GraphCache evicted the oldest entry first and then overwrote A's
    slot; with A the younger entry that threw B out, and this test failed.)"""
    for first_is_a in (True, False):
        c, build = GraphCache(size=2), Builder()
        ea, eb = edges(), edges()
        if first_is_a:
            a, b = c.get((ea,), 3, build), c.get((eb,), 3, build)
        else:
            b, a = c.get((eb,), 3, build), c.get((ea,), 3, build)
        ea[0, 0] = 2
        a2 = c.get((ea,), 3, build)
        assert a2 is not a and build.calls == 3
        assert c.get((eb,), 3, build) is b and build.calls == 3
        assert c.get((ea,), 3, build) is a2 and build.calls == 3


def test_a_failed_build_changes_nothing():
    c, build = GraphCache(size=2), Builder()
    e1, e2, e3 = edges(), edges(), edges()
    a, b = c.get((e1,), 3, build), c.get((e2,), 3, build)

    def fails():
        raise IndexError("edge_index out of range")
    try:
        c.get((e3,), 3, fails)
    except IndexError:
        pass
    assert c.get((e1,), 3, build) is a and c.get((e2,), 3, build) is b and build.calls == 2


def test_the_entry_holds_its_tensors():
    c, build = GraphCache(), Builder()
    ei = edges()
    ref, key = weakref.ref(ei), id(ei)
    a = c.get((ei,), 3, build)
    del ei
    gc.collect()
    assert ref() is not None and id(ref()) == key                      # alive: no new tensor can take this id
    assert c.get((ref(),), 3, build) is a and build.calls == 1
    c.get((edges(),), 3, build)
    c.get((edges(),), 3, build)                                        # two new keys: the first entry is evicted
    gc.collect()
    assert ref() is None                                               # ... and with it the tensor it held
