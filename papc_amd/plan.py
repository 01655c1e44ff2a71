"""The sampling plan of one set-abstraction level: its layout as a flat tuple of device tensors, written down once.

``sample()`` of a layer returns the weight-independent half of that level (FPS, ball query, SA1's grouped coordinates, the compact plan, the
point lists) as a FLAT tuple, and ``forward(sampled=)`` / ``sample(out=)`` take one back -- possibly a copy that kept nothing but the tensors:

    SSG level:  new_xyz, idx
                [, xc, gram]                         coordinates-only first layer (mlp.xyz_pregroup)
              | [, 7 compact tensors][, 3 list tensors]
    MSG level:  new_xyz, idx_0 .. idx_{R-1}, then per branch in order: [7 compact tensors [, 3 list tensors]]

(the 7: ``compact.CompactPlan.tensors()``, the 3: ``compact.PointLists.tensors()``).  An SSG layout is decided by the tuple's length; an MSG
layout by R, by which branches the layer runs compacted, and by ``compact.is_lists`` on the three tensors after a branch's compact plan.

The contract with the callers that see the tuple itself -- no marker objects in it, its length and order as above:
  * ``bench.py`` reads a compacted SSG level as ``len(pl2) in (9, 12)`` and its row count as ``pl2[4]`` (``CompactPlan.rows``);
  * ``bench.py`` walks a level with ``for t in lvl`` (``record_stream``, ``clone``): every element is a tensor;
  * ``models.*.plan_sampling(..., out=, stage=)`` hands a previous result back as ``out`` and writes the centroids into ``out[0][0]``.
"""
from .compact import CompactPlan, PointLists, alloc, alloc_lists, is_lists

N_COMPACT = len(CompactPlan(alloc(1, 1, "cpu"), 1, 1).tensors())
N_LISTS = len(PointLists(alloc_lists(1, 1, 1, 1, "cpu"), False).tensors())
N_XYZ_PRE = 2            # (xc, gram) of mlp.xyz_pregroup


def new_xyz(flat):
    """the centroids [B, S, 3] of a level's flat plan"""
    return flat[0]


class Level:
    """structured view of a level's plan: new_xyz, idxs[i], xyz_pre = (xc, gram) | None, cplans[i] = CompactPlan | None,
    plists[i] = PointLists | None (i = radius branch; an SSG level has one)"""
    __slots__ = ("new_xyz", "idxs", "xyz_pre", "cplans", "plists")

    def __init__(self, new_xyz, idxs, xyz_pre=None, cplans=None, plists=None):
        self.new_xyz, self.idxs, self.xyz_pre = new_xyz, list(idxs), xyz_pre
        self.cplans, self.plists = list(cplans or [None] * len(self.idxs)), list(plists or [None] * len(self.idxs))

    def branch(self, i):
        """the plan tensors of branch i beyond its index lists"""
        return tuple(t for p in (self.cplans[i], self.plists[i]) if p is not None for t in p.tensors())

    def flat(self):
        return sum((self.branch(i) for i in range(len(self.idxs))), (self.new_xyz, *self.idxs, *(self.xyz_pre or ())))

    @classmethod
    def parse(cls, flat, G, nsamples, compacted=None):
        """``flat`` = a ``sample()`` result (any sequence of its tensors); G = B * S groups; nsamples = K per branch; ``compacted`` = per
        branch whether the layer runs it compacted (MSG), None = an SSG level, whose length tells"""
        flat = tuple(flat)
        pos = 1 + len(nsamples)
        n = len(flat) - pos
        lv = cls(flat[0], flat[1:pos])
        if compacted is None and n == N_XYZ_PRE:
            lv.xyz_pre, pos = flat[pos:], len(flat)
        compacted = [n >= N_COMPACT] if compacted is None else compacted
        for i, K in enumerate(nsamples):
            if compacted[i] and len(flat) >= pos + N_COMPACT:
                lv.cplans[i] = CompactPlan(flat[pos:pos + N_COMPACT], G, K)
                pos += N_COMPACT
            # (the lists are recognised by what they are, not by the layer's current mode: a plan made in another mode parses all the same)
            if is_lists(flat[pos:pos + N_LISTS]):
                lv.plists[i] = PointLists(flat[pos:pos + N_LISTS], lv.cplans[i] is not None)
                pos += N_LISTS
        if n < 0 or pos != len(flat):
            raise ValueError("a sampling plan of %d tensors is no layout of this level (%d index lists, compacted branches %s: %d tensors expected)"
                             % (len(flat), len(nsamples), list(compacted), pos))
        return lv


class Cursor:
    """Writes a level's flat plan piece by piece over an optional ``out`` -- a previous result for the same shapes the kernels fill in place.
    ``next(n)`` = the buffers of the next n tensors, or None; ``put`` appends what was made of them."""

    def __init__(self, out):
        self.out = None if out is None else tuple(out)
        self.res = ()

    def next(self, n, then=None):
        """out's n tensors at the current position; None without ``out``, with fewer left, or unless ``then`` holds the count left after them"""
        left = -1 if self.out is None else len(self.out) - len(self.res) - n
        return self.out[len(self.res):len(self.res) + n] if left >= 0 and (then is None or left in then) else None

    def put(self, *tensors):
        self.res += tensors
        return self.res
