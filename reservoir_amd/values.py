"""``RandomValues`` (Sampler.scala:383-412) over arbitrary hashable elements, in pure Python.

The host half of ``Sampler.distinct`` for any ``B`` (``key_type="object"``): the engine's hash-only
candidate pass returns the few elements the reference could still admit, and this replica decides
them exactly as the reference does -- a max-heap on the scrambled hash, a set of the elements, and
``maxHash``.  No GPU dependency.

The heap is scala 2.13's ``mutable.PriorityQueue`` (1-indexed array), whose tie order decides which
members of an oversubscribed boundary hash bucket stay (reservoir_amd/csrc/rsv_host_values.h states
the same order): ``fixUp`` swaps while parent < child; ``fixDown`` takes the larger child, the left
one on ties, and stops when parent >= child.
"""
from __future__ import annotations

LONG_MIN = -(2**63)


class RandomValues:
    """``sample(elem, h)`` is RandomValues.sample (Sampler.scala:394-409) for an element already
    mapped, with its scrambled hash ``h`` (Sampler.scala:396)."""

    def __init__(self, max_sample_size: int):
        if max_sample_size <= 0:
            raise ValueError("maxSampleSize must be positive")
        self._k = int(max_sample_size)
        self._h = [LONG_MIN]  # slot 0 unused: the queue is 1-indexed
        self._e = [None]
        self._elements = set()
        self.max_hash = LONG_MIN  # Sampler.scala:392

    @property
    def size(self) -> int:
        return len(self._h) - 1

    def _enqueue(self, elem, h) -> None:  # addOne + fixUp
        H, E = self._h, self._e
        H.append(h)
        E.append(elem)
        m = len(H) - 1
        while m > 1 and H[m >> 1] < h:
            H[m], E[m] = H[m >> 1], E[m >> 1]
            m >>= 1
        H[m], E[m] = h, elem

    def _dequeue(self):  # the head leaves, the last entry sinks from the root (fixDown)
        H, E = self._h, self._e
        res = E[1]
        h, e = H.pop(), E.pop()
        n = len(H) - 1
        if n == 0:
            return res
        k = 1
        while 2 * k <= n:
            j = 2 * k
            if j < n and H[j] < H[j + 1]:
                j += 1
            if h >= H[j]:
                break
            H[k], E[k] = H[j], E[j]
            k = j
        H[k], E[k] = h, e
        return res

    def sample(self, elem, h: int) -> None:
        if self.size < self._k:
            if elem not in self._elements:
                self._enqueue(elem, h)
                self._elements.add(elem)
                if h > self.max_hash:
                    self.max_hash = h
        elif h < self.max_hash and elem not in self._elements:
            self._elements.discard(self._dequeue())
            self._enqueue(elem, h)
            self._elements.add(elem)
            self.max_hash = self._h[1]

    def admits(self, elem, h: int) -> bool:
        """Whether ``sample(elem, h)`` would change the set."""
        if self.size < self._k:
            return elem not in self._elements
        return h < self.max_hash and elem not in self._elements

    def __contains__(self, elem) -> bool:
        return elem in self._elements

    def heap(self):
        """``(elements, hashes)`` in the queue's array order: entry j of the 1-indexed queue at index j - 1.
        New lists; the sampler is left as it is."""
        return self._e[1:], self._h[1:]

    def result(self) -> list:
        """The set's elements, ascending by scrambled hash (the reference's order is HashSet order)."""
        order = sorted(range(1, len(self._h)), key=self._h.__getitem__)
        return [self._e[i] for i in order]

    def hashes(self) -> list:
        return sorted(self._h[1:])
