"""A reference for what a bounding-volume tree COSTS the rays that walk it, in plain numpy and float64, written from the
literature and not from the project's builder: a top-down binary tree split by the surface-area heuristic with a full sweep over
the three centroid axes (Goldsmith and Salmon 1987; MacDonald and Booth 1990; the sweep as in Wald 2007), the tree a broken sort
would give (median splits over a random order), a greedy 4-wide collapse (Wald, Benthin and Boulos 2008: a node adopts the
children of its largest child), and an ordered closest-hit walk that counts what the walk fetches.

The units are those of ptx_trace_rays' diagnostic mode 2: one visit per wide node fetched, one test per triangle tested.  The
numbers are not the HIP tree's numbers (other boxes, other collapse, pair leaves): they are the two ends of a scale -- what a good
tree and what a tree without spatial order cost on the same rays -- between which a builder's result is judged."""
import numpy as np

EMPTY = np.int64(-(1 << 62))  # a child slot that holds nothing


def live_mask(tris):
    """Triangles whose float32 edge cross product does not vanish (the rule of test_tree_adversarial.live_mask): the others
    have no area and are in no tree."""
    w = np.float32(tris)
    return (np.cross(w[:, 1] - w[:, 0], w[:, 2] - w[:, 0]) != 0).any(axis=1)


def _area(lo, hi):
    d = np.maximum(hi - lo, 0.0)
    return d[..., 0] * d[..., 1] + d[..., 1] * d[..., 2] + d[..., 2] * d[..., 0]


class BinaryTree:
    """Nodes 0 .. m-1, root 0.  left / right: a node index (>= 0) or ~k for the leaf of triangle `tri_ids[k]`.  tris: the float64
    triangles of the leaves, tri_ids their indices in the array the tree was built from."""

    def __init__(self, tris, tri_ids):
        self.tris, self.tri_ids = tris, tri_ids
        self.left, self.right, self.lo, self.hi = [], [], [], []

    def add(self, lo, hi):
        self.left.append(0)
        self.right.append(0)
        self.lo.append(lo)
        self.hi.append(hi)
        return len(self.left) - 1


def _prepare(tris):
    tris = np.asarray(tris)
    ids = np.flatnonzero(live_mask(tris))
    T = np.float64(tris[ids])
    return T, ids, T.min(axis=1), T.max(axis=1)


def _sah_split(idx, tlo, thi, cen, axes):
    """The cheapest of the len(idx) - 1 cuts of the sorted order along each axis: area(left) * count(left) + area(right) *
    count(right).  Returns (left indices, right indices)."""
    n = len(idx)
    best = (np.inf, None, None)
    counts = np.arange(1, n, dtype=np.float64)
    for ax in axes:
        order = idx[np.argsort(cen[idx, ax], kind="stable")]
        lo, hi = tlo[order], thi[order]
        left = _area(np.minimum.accumulate(lo, axis=0), np.maximum.accumulate(hi, axis=0))[:-1]
        right = _area(np.minimum.accumulate(lo[::-1], axis=0), np.maximum.accumulate(hi[::-1], axis=0))[::-1][1:]
        cost = left * counts + right * counts[::-1]
        k = int(np.argmin(cost))
        if cost[k] < best[0]:
            best = (cost[k], order, k + 1)
    return best[1][:best[2]], best[1][best[2]:]


def build_sah(tris, axes=(0, 1, 2)):
    """Top-down binary tree over the live triangles, every inner node split at the cheapest cut of a full surface-area sweep
    over the centroid axes `axes`; one triangle per leaf."""
    T, ids, tlo, thi = _prepare(tris)
    tree = BinaryTree(T, ids)
    if len(T) < 2:
        return tree
    cen = T.mean(axis=1)
    root = tree.add(tlo.min(axis=0), thi.max(axis=0))
    todo = [(root, np.arange(len(T)))]
    while todo:
        node, idx = todo.pop()
        halves = _sah_split(idx, tlo, thi, cen, axes)
        for side, part in zip(("left", "right"), halves):
            if len(part) == 1:
                ref = ~int(part[0])
            else:
                ref = tree.add(tlo[part].min(axis=0), thi[part].max(axis=0))
                todo.append((ref, part))
            getattr(tree, side)[node] = ref
    return tree


def build_scrambled(tris, seed):
    """The tree a sort that does not sort would give: the live triangles in a seeded random order, split at the median index,
    the boxes fitted to what each half holds.  A valid tree with no spatial order."""
    T, ids, tlo, thi = _prepare(tris)
    tree = BinaryTree(T, ids)
    if len(T) < 2:
        return tree
    order = np.random.default_rng(seed).permutation(len(T))
    root = tree.add(tlo.min(axis=0), thi.max(axis=0))
    todo = [(root, order)]
    while todo:
        node, idx = todo.pop()
        halves = (idx[:len(idx) // 2], idx[len(idx) // 2:])
        for side, part in zip(("left", "right"), halves):
            if len(part) == 1:
                ref = ~int(part[0])
            else:
                ref = tree.add(tlo[part].min(axis=0), thi[part].max(axis=0))
                todo.append((ref, part))
            getattr(tree, side)[node] = ref
    return tree


class WideTree:
    """child (m, 4): a wide node index (>= 0), ~k for the leaf of triangle k, or EMPTY; lo / hi (m, 4, 3): the children's boxes
    (an empty slot has the box no ray enters).  Root 0; m == 0: no triangles."""

    def __init__(self, tris, tri_ids, child, lo, hi):
        self.tris, self.tri_ids, self.child, self.lo, self.hi = tris, tri_ids, child, lo, hi


def collapse4(tree):
    """4-wide nodes by the plain greedy rule: a node starts with its two children and, while it has fewer than four, replaces
    its inner child of the largest surface area by that child's two children."""
    T = tree.tris
    tlo, thi = T.min(axis=1), T.max(axis=1)
    if len(T) == 0:
        return WideTree(T, tree.tri_ids, np.zeros((0, 4), np.int64), np.zeros((0, 4, 3)), np.zeros((0, 4, 3)))
    if len(T) == 1:
        child = np.array([[~0, EMPTY, EMPTY, EMPTY]], np.int64)
        lo, hi = np.full((1, 4, 3), np.inf), np.full((1, 4, 3), -np.inf)
        lo[0, 0], hi[0, 0] = tlo[0], thi[0]
        return WideTree(T, tree.tri_ids, child, lo, hi)
    nlo, nhi = np.array(tree.lo), np.array(tree.hi)
    narea = _area(nlo, nhi)
    child, lo, hi = [], [], []
    wide_of = {0: 0}
    todo = [0]
    child.append(None)
    while todo:
        b = todo.pop()
        kids = [tree.left[b], tree.right[b]]
        while len(kids) < 4:
            inner = [k for k in kids if k >= 0]
            if not inner:
                break
            big = max(inner, key=lambda k: narea[k])
            at = kids.index(big)
            kids[at:at + 1] = [tree.left[big], tree.right[big]]
        row = []
        for k in kids:
            if k >= 0:
                wide_of[k] = len(child)
                child.append(None)
                todo.append(k)
                row.append((wide_of[k], nlo[k], nhi[k]))
            else:
                row.append((k, tlo[~k], thi[~k]))
        row += [(EMPTY, np.full(3, np.inf), np.full(3, -np.inf))] * (4 - len(row))
        child[wide_of[b]] = row
    m = len(child)
    out = WideTree(T, tree.tri_ids, np.zeros((m, 4), np.int64), np.zeros((m, 4, 3)), np.zeros((m, 4, 3)))
    for w, row in enumerate(child):
        for k, (ref, l, h) in enumerate(row):
            out.child[w, k], out.lo[w, k], out.hi[w, k] = ref, l, h
    return out


def _triangle_test(T, o, d, tmin, tmax):
    """Moeller and Trumbore 1997 in float64, row by row: t where the ray meets its triangle inside (tmin, tmax), inf elsewhere."""
    v0, e1, e2 = T[:, 0], T[:, 1] - T[:, 0], T[:, 2] - T[:, 0]
    p = np.cross(d, e2)
    det = np.einsum("ij,ij->i", e1, p)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / det
        s = o - v0
        u = np.einsum("ij,ij->i", s, p) * inv
        q = np.cross(s, e1)
        v = np.einsum("ij,ij->i", d, q) * inv
        t = np.einsum("ij,ij->i", e2, q) * inv
        ok = (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > tmin) & (t < tmax)
    return np.where(ok, t, np.inf)


def count(tree, rays):
    """An ordered closest-hit walk of every ray (8 floats: origin, tmin, direction, tmax) through a WideTree: a node's children
    whose boxes the ray enters before its best hit are taken nearest first, the others wait on a stack with their entry
    distance and are dropped when the best hit has come nearer than that.  A hit counts for tmin < t < tmax; equal t goes to
    the smaller triangle index.  Returns (wide nodes fetched, triangles tested, hit triangle or -1, t or inf) per ray.  All rays
    advance together, one stack entry each per round."""
    rays = np.float64(np.asarray(rays).reshape(-1, 8))
    n = len(rays)
    visits, tests = np.zeros(n, np.int64), np.zeros(n, np.int64)
    hit, best = np.full(n, -1, np.int64), np.full(n, np.inf)
    if n == 0 or len(tree.child) == 0:
        return visits, tests, hit, best
    o, d, tmin, tmax = rays[:, 0:3], rays[:, 4:7], rays[:, 3], rays[:, 7]
    with np.errstate(divide="ignore"):
        inv = 1.0 / np.where(d == 0, np.copysign(1e-300, d), d)  # 0 * inf has no place in a slab test
    ok = np.isfinite(rays).all(axis=1) & (d != 0).any(axis=1) & (tmax > tmin)
    limit = tmax.copy()                                # the walk looks for hits below this: tmax, then the best t
    ref = np.zeros((n, 64), np.int64)                  # per ray: stack of references ...
    near = np.zeros((n, 64))                           # ... and the distance at which the ray enters each
    sp = np.where(ok, 1, 0)
    act = np.flatnonzero(sp > 0)
    while len(act):
        sp[act] -= 1
        r, e = ref[act, sp[act]], near[act, sp[act]]
        keep = e < limit[act]                          # still nearer than the best hit?
        a, r = act[keep], r[keep]
        leaf = r < 0
        if leaf.any():
            al, k = a[leaf], ~r[leaf]
            tests[al] += 1
            t = _triangle_test(tree.tris[k], o[al], d[al], tmin[al], tmax[al])
            gid = tree.tri_ids[k]
            better = (t < best[al]) | ((t == best[al]) & np.isfinite(t) & (gid < hit[al]))
            best[al[better]], hit[al[better]] = t[better], gid[better]
            limit[al[better]] = t[better]
        if (~leaf).any():
            an, w = a[~leaf], r[~leaf]
            visits[an] += 1
            with np.errstate(invalid="ignore"):
                t0 = (tree.lo[w] - o[an, None]) * inv[an, None]
                t1 = (tree.hi[w] - o[an, None]) * inv[an, None]
            tn = np.maximum(np.minimum(t0, t1).max(axis=2), tmin[an, None])
            tf = np.minimum(np.maximum(t0, t1).min(axis=2), limit[an, None])
            entered = (tn <= tf) & (tn < limit[an, None]) & (tree.child[w] != EMPTY)  # (NaN compares false: an empty slot)
            tn = np.where(entered, tn, np.inf)
            order = np.argsort(tn, axis=1, kind="stable")
            if sp[an].max() + 4 > ref.shape[1]:
                ref = np.concatenate([ref, np.zeros_like(ref)], axis=1)
                near = np.concatenate([near, np.zeros_like(near)], axis=1)
            rows = np.arange(len(an))
            for slot in (3, 2, 1, 0):                  # farthest first, so that the nearest is on top
                c = order[:, slot]
                push = entered[rows, c]
                ap = an[push]
                ref[ap, sp[ap]], near[ap, sp[ap]] = tree.child[w[push], c[push]], tn[rows[push], c[push]]
                sp[ap] += 1
        act = act[sp[act] > 0]
    return visits, tests, hit, best


def mean_cost(tree, rays):
    """Mean of visits + tests per ray."""
    v, t, _, _ = count(tree, rays)
    return float((v + t).mean())


def quality_rays(tris, lo, hi, n, seed):
    """n rays (float32, 8 each, tmin 1e-5, tmax 1e4) against which a tree is priced.  The first half: origins uniform in the
    box [lo, hi]^3, directions uniform on the sphere (what util.random_rays draws).  The other half, what most rays of a
    path tracer are: from the centroid of a seeded random live triangle, on either side of it, cosine-distributed about the
    normal of that side.  The origin is lifted off the triangle by 1e-4 of the box, as a renderer offsets the rays it spawns,
    so that no ray grazes the surface it starts from at a distance where float32 and float64 disagree about tmin.  The two
    kinds alternate, so that any leading part of the rays is a sample of both."""
    rng = np.random.default_rng(seed)
    rays = np.zeros((n, 8), np.float32)
    rays[:, 3], rays[:, 7] = 1e-5, 1e4
    m = n // 2
    rays[:m, 0:3] = rng.uniform(lo, hi, size=(m, 3))
    u = rng.normal(size=(m, 3))
    rays[:m, 4:7] = u / np.linalg.norm(u, axis=1, keepdims=True)
    T = np.float64(np.asarray(tris)[live_mask(tris)])
    if len(T) == 0:
        return rays[:m]
    pick = T[rng.integers(0, len(T), n - m)]
    nrm = np.cross(pick[:, 1] - pick[:, 0], pick[:, 2] - pick[:, 0])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm *= rng.choice([-1.0, 1.0], size=(n - m, 1))
    # cosine-distributed: a uniform point of the unit disc lifted onto the hemisphere (Malley's method)
    rad, phi = np.sqrt(rng.uniform(size=n - m)), rng.uniform(0, 2 * np.pi, n - m)
    helper = np.where(np.abs(nrm[:, 0:1]) < 0.9, [[1.0, 0.0, 0.0]], [[0.0, 1.0, 0.0]])
    tx = np.cross(nrm, helper)
    tx /= np.linalg.norm(tx, axis=1, keepdims=True)
    ty = np.cross(nrm, tx)
    w = (rad * np.cos(phi))[:, None] * tx + (rad * np.sin(phi))[:, None] * ty + np.sqrt(np.maximum(1.0 - rad * rad, 0.0))[:, None] * nrm
    rays[m:, 0:3] = pick.mean(axis=1) + nrm * (1e-4 * (hi - lo))
    rays[m:, 4:7] = w / np.linalg.norm(w, axis=1, keepdims=True)
    out = np.empty_like(rays)
    out[0:2 * m:2], out[1:2 * m:2], out[2 * m:] = rays[:m], rays[m:2 * m], rays[2 * m:]
    return out
