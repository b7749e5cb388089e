"""hybridneuralrendering_amd/_cache.py on CPU tensors (an address and a version counter exist there too): the key sees every way a source can
change, the entry keeps its sources alive, `mark_written` reaches the entry through views -- and no other file of the package spells the key."""
import os
import re

import torch

from hybridneuralrendering_amd._cache import Derived, mark_written, tensor_key


class _Counter:
    def __init__(self):
        self.n = 0

    def __call__(self):
        self.n += 1
        return self.n


def test_a_hit_on_the_same_tensors_and_a_miss_for_every_way_a_source_changes():
    a, b = torch.arange(12.0), torch.ones(3)
    e, build = Derived(), _Counter()
    assert e.key is None and e.value is None
    assert e.get([a, b], build) == 1 and e.get([a, b], build) == 1 and e.get((a, b), build) == 1 and build.n == 1
    assert e.value == 1 and e.key == (tensor_key([a, b]), ())
    a.add_(1)                                                                   # the version counter
    assert e.get([a, b], build) == 2 and e.get([a, b], build) == 2
    assert e.get([a.clone(), b], build) == 3                                    # the address
    assert e.get([a, b], build) == 4
    v = a.view(3, 4)                                                            # the shape, at the same address and version
    assert v.data_ptr() == a.data_ptr() and v._version == a._version
    assert e.get([v, b], build) == 5 and e.get([v, b], build) == 5
    assert e.get([v, b], build, extra=(3, 3, 3)) == 6 and e.get([v, b], build, extra=(3, 3, 3)) == 6      # the rest of the key
    assert e.get([v, b], build, extra=(3, 3, 1)) == 7
    assert e.get([v], build, extra=(3, 3, 1)) == 8                              # the number of sources
    assert build.n == 8


def test_mark_written_is_a_miss_also_through_a_view():
    a = torch.zeros(8)
    e, build = Derived(), _Counter()
    e.get([a], build)
    mark_written([a])
    assert e.get([a], build) == 2
    mark_written([a[2:6]])                                                      # a view shares its base's counter
    assert e.get([a], build) == 3
    half = a[:4]
    e.get([half], build)
    mark_written(t for t in [a])                                                # ... in both directions; any iterable
    assert e.get([half], build) == 5 and e.get([half], build) == 5


def test_sources_unchanged_follows_in_place_writes_to_a_held_source():
    a, b = torch.zeros(4), torch.zeros(2)
    e = Derived()
    assert not e.sources_unchanged()                                            # an empty entry has no sources to vouch for
    e.get([a, b], lambda: "v")
    assert e.sources_unchanged()
    torch.zeros(4).add_(1)                                                      # (another tensor's write is not its business)
    e.get([a, b], lambda: "w")
    assert e.sources_unchanged() and e.value == "v"
    b.mul_(2)
    assert not e.sources_unchanged()
    e.get([a, b], lambda: "w")
    assert e.sources_unchanged() and e.value == "w"
    mark_written([a])
    assert not e.sources_unchanged()


def test_build_still_sees_the_old_entry():
    a = torch.zeros(4)
    e = Derived()
    e.get([a], lambda: "old")
    a.add_(1)
    seen = []
    e.get([a], lambda: seen.append((e.value, e.sources_unchanged())) or "new")
    assert seen == [("old", False)] and e.value == "new" and e.sources_unchanged()


def test_the_entry_keeps_its_sources_alive():
    a = torch.full((1000,), 7.0)
    ptr = a.data_ptr()
    e = Derived()
    e.get([a], lambda: 0)
    del a
    held = e.sources[0]
    assert held.data_ptr() == ptr and bool((held == 7.0).all())
    junk = [torch.empty(1000) for _ in range(8)]                                # nothing new lands on the held address
    assert all(t.data_ptr() != ptr for t in junk) and e.sources_unchanged()
    e.invalidate()
    assert e.sources == ()


def test_invalidate_forces_a_rebuild_and_so_does_assigning_none_to_the_key():
    a = torch.zeros(4)
    e, build = Derived(), _Counter()
    e.get([a], build)
    e.invalidate()
    assert e.key is None and e.value is None
    assert e.get([a], build) == 2
    e.key = None
    assert e.value is None and e.get([a], build) == 3
    e.key = ("stale",)                                                          # any other key is simply stored (and is a miss)
    assert e.key == ("stale",) and not e.sources_unchanged() and e.get([a], build) == 4


def test_a_failed_build_leaves_the_entry_as_it_was():
    a = torch.zeros(4)
    e = Derived()
    e.get([a], lambda: "v")
    a.add_(1)
    try:
        e.get([a], lambda: 1 // 0)
    except ZeroDivisionError:
        pass
    assert e.value == "v" and not e.sources_unchanged() and e.get([a], lambda: "w") == "w"


# docstrings that may MENTION the counter by name, by file (none today: they all point to _cache.py)
_MAY_MENTION = {}


def test_only_cache_py_spells_the_key_or_bumps_a_version():
    """The next derived value goes through _cache.py too: no other file of the package reads a tensor's version counter or bumps one."""
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hybridneuralrendering_amd")
    pat = re.compile(r"(?<![A-Za-z0-9_])_version\b|increment_version")
    found = {}
    for root, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                n = len(pat.findall(open(os.path.join(root, f)).read()))
                if n:
                    found[os.path.relpath(os.path.join(root, f), pkg)] = n
    assert found.pop("_cache.py", 0) > 0
    assert found == _MAY_MENTION
