"""`PendingOutputs`: the output dict of a forward whose head maps (all but the heat map) were computed at the peaks only
(model.heads_at_peaks, plan._Plan.run).  It is a dict with the keys and the order of the dense forward; the FIRST read of a
value through the public mapping interface - `[]`, `get`, `pop`, `items`, `values`, iteration, `dict(y)`, `copy`, `==` - calls
the materialiser once, which runs the dense head launches into the very tensors the dict holds, and from then on it is an
ordinary dict.  Key queries (`in`, `len`, `keys`) and writes do not materialise.  decode.py reads through `peek`, which never
does: the decoder needs the maps at the peaks alone."""
import threading


class PendingOutputs(dict):
    __slots__ = ("_materialiser", "_release", "_lock", "__weakref__")

    def __init__(self, items, materialiser, lock=None, release=None):
        """lock: the lock the materialiser's launches need (the model's: a forward releases unread outputs while it holds it, so
        a reader must take that lock and no other, or the two could wait for each other).  release: makes the materialiser
        independent of buffers its owner is about to overwrite (None: there is no such way - `release` then materialises)."""
        dict.__init__(self, items)
        self._materialiser = materialiser
        self._release = release
        self._lock = lock if lock is not None else threading.RLock()

    # ------------------------------------------------------------------------------------------ state
    @property
    def pending(self):
        return self._materialiser is not None

    def materialise(self):
        """Run the dense launches if they have not run yet (once; a failing materialiser leaves the dict pending)."""
        if self._materialiser is None:
            return
        with self._lock:
            m = self._materialiser
            if m is not None:
                m()
                self._materialiser = self._release = None

    def release(self):
        """Called by the owner before it reuses what the materialiser reads (once; nothing to do once the maps are complete)."""
        with self._lock:
            r = self._release
            if self._materialiser is None or r is False:   # (complete, or released before)
                return
            if r is not None:
                r()
                self._release = False
                return
        self.materialise()

    # ------------------------------------------------------------------------------------------ private access (decode.py)
    def peek(self, key, default=None):
        """the value under `key` WITHOUT materialising: valid at the forward's peaks only while the dict is pending"""
        return dict.get(self, key, default)

    def rename(self, old, new):
        """`self[new] = self.pop(old)` without materialising (fusionDecode's `rotation2` -> `rotation`)"""
        dict.__setitem__(self, new, dict.pop(self, old))

    # ------------------------------------------------------------------------------------------ reads materialise
    def __getitem__(self, key):
        self.materialise()
        return dict.__getitem__(self, key)

    def get(self, key, default=None):
        self.materialise()
        return dict.get(self, key, default)

    def pop(self, *args):
        self.materialise()
        return dict.pop(self, *args)

    def popitem(self):
        self.materialise()
        return dict.popitem(self)

    def setdefault(self, key, default=None):
        self.materialise()
        return dict.setdefault(self, key, default)

    def items(self):
        self.materialise()
        return dict.items(self)

    def values(self):
        self.materialise()
        return dict.values(self)

    def copy(self):
        self.materialise()
        return dict(dict.items(self))

    def __eq__(self, other):
        self.materialise()
        return dict.__eq__(self, other)

    def __ne__(self, other):
        self.materialise()
        return dict.__ne__(self, other)

    __hash__ = None

    # CPython copies a dict subclass's storage directly - no __getitem__ - in dict(y) / {**y} / d.update(y) unless __iter__ is
    # overridden; with it (and keys) they go through keys() and __getitem__, which materialises
    def __iter__(self):
        self.materialise()
        return dict.__iter__(self)

    def keys(self):
        return dict.keys(self)

    # (these go to the dict's storage directly, too)
    def __repr__(self):
        self.materialise()
        return dict.__repr__(self)

    def __or__(self, other):
        self.materialise()
        return dict.__or__(self, other)

    def __ror__(self, other):
        self.materialise()
        return dict.__ror__(self, other)

    def __ior__(self, other):
        self.materialise()
        dict.update(self, other)
        return self

    def __reduce__(self):
        self.materialise()
        return (dict, (dict(dict.items(self)),))
