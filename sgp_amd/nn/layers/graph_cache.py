"""The cache behind every per-graph plan."""


class GraphCache:
    """What ``build()`` made for the last ``size`` graphs, keyed by the identity of ``tensors`` and by ``extra``.

    An entry keeps its tensors, so an ``id`` in a live key cannot pass to another object.  A tensor written in place
    since (``_version``) rebuilds its entry where it stands; only a new key evicts, oldest inserted first."""

    def __init__(self, size=2):
        self._d, self._size = {}, size

    def get(self, tensors, extra, build):
        """``tensors``: a tuple of tensors or ``None``; ``extra``: hashable, such as ``(n, str(device))``."""
        key = (tuple(None if t is None else id(t) for t in tensors), extra)
        ver = tuple(0 if t is None else t._version for t in tensors)
        hit = self._d.get(key)
        if hit is None or hit[1] != ver:
            value = build()
            if hit is None and len(self._d) >= self._size:
                self._d.pop(next(iter(self._d)))
            hit = (tensors, ver, value)
            self._d[key] = hit
        return hit[2]
