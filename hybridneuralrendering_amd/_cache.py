"""Values derived from device tensors, cached: packed weights, the reference views' feature map, the per-point table, the point records, the voxel grid.

Three rules make such a cache safe, and they live here and nowhere else:

1. The key holds the address, shape, in-place version counter and device of EVERY source tensor (`tensor_key`) -- `load_state_dict`, optimiser steps,
   `.to()` and any other in-place update are seen through them -- plus whatever else the value depends on (`extra`: option tuples, another entry's key).
2. The sources stay referenced while the entry lives (`Derived.sources`): the caching allocator hands a freed buffer's address, at version 0, to
   the next tensor of that size, which would look like a hit.  A tensor swapped in through `p.data = other` escapes this: `invalidate()` after it.
3. A kernel that writes a tensor behind torch's back leaves `tensor._version` where it was, so whoever launches it calls `mark_written` on what it
   wrote -- DeviceAdam.step (`mark_updated()` after a graph replay that contains the step), BatchSampler.next, PathSampler.next.  Without the mark the
   next evaluation silently uses the value derived from the old contents.  A captured graph replays the kernel, not the mark: whoever replays it marks.
"""
import torch


def tensor_key(tensors):
    return tuple((t.data_ptr(), t.shape, t._version, t.device) for t in tensors)


def mark_written(tensors):
    """Rule 3: every tensor counts as modified in place (a view marks its base, and the other way round)."""
    for t in tensors:
        torch.autograd.graph.increment_version(t)


class Derived:
    """One cached value: `key` = (tensor_key of `sources`, extra) and `value`; an empty entry has key None.  Assigning None to `key` empties it."""

    def __init__(self):
        self.invalidate()

    def invalidate(self):
        self._key, self.value, self.sources = None, None, ()

    @property
    def key(self):
        return self._key

    @key.setter
    def key(self, key):
        if key is None:
            self.invalidate()
        else:
            self._key = key

    def get(self, tensors, build, extra=()):
        """The value for these sources and `extra`; `build()` makes it on a miss, and still sees the old entry while it runs."""
        tensors = tuple(tensors)
        key = (tensor_key(tensors), extra)
        if key != self._key:
            self.value = build()
            self._key, self.sources = key, tensors
        return self.value

    def sources_unchanged(self):
        """True when the tensors the value was built from are still what they were then: such an entry may be extended instead of rebuilt."""
        return self._key is not None and tensor_key(self.sources) == self._key[0]
