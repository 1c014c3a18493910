"""Host-side checker of a read-back render tree (Device.read_bvh; the byte
layouts are in include/ptgpu.h under pt_debug_read_bvh).  numpy only.

Every check_* function returns a list of violations, each a string that
starts with the name of the rule it breaks ("topology: ...", "leaves: ...",
"containment: ...", "stack: ...", "order: ..."); an empty list is a sound tree.
Boxes and primitives are compared in float64 from the float32 values the
kernel reads, without tolerance."""
import numpy as np

MAX_REPORT = 20  # violations listed per rule (the count is always given)


def refs4(nodes4):
    return np.ascontiguousarray(nodes4[:, 24:28]).view(np.int32)


def boxes4(nodes4):
    """(n4, 4 slots, 3 axes) float64 lo and hi."""
    f = nodes4.astype(np.float64)
    lo = np.stack([f[:, 0:4], f[:, 8:12], f[:, 16:20]], axis=2)
    hi = np.stack([f[:, 4:8], f[:, 12:16], f[:, 20:24]], axis=2)
    return lo, hi


def refs2(nodes2):
    return np.ascontiguousarray(nodes2[:, 12:14]).view(np.int32)


def boxes2(nodes2):
    """(n2, 2 children, 3 axes) float64 lo and hi."""
    f = nodes2.astype(np.float64)
    lo = np.stack([np.stack([f[:, 0], f[:, 2], f[:, 8]], 1), np.stack([f[:, 4], f[:, 6], f[:, 10]], 1)], 1)
    hi = np.stack([np.stack([f[:, 1], f[:, 3], f[:, 9]], 1), np.stack([f[:, 5], f[:, 7], f[:, 11]], 1)], 1)
    return lo, hi


def decode(cur):
    c = ~int(cur)
    return c >> 3, (c & 7) + 1


def cursor(first, count):
    return ~((int(first) << 3) | (int(count) - 1))


def is_triangle(prims):
    return (np.ascontiguousarray(prims[:, 3]).view(np.int32) & 1) == 1


def prim_extent(prims):
    """Per primitive, the box of what the kernel tests, in float64: v0, v0+e1,
    v0+e2 of a triangle, c - r and c + r of a sphere."""
    p = prims.astype(np.float64)
    v0, e1, e2 = p[:, 0:3], p[:, 4:7], p[:, 8:11]
    tri = is_triangle(prims)[:, None]
    r = np.abs(p[:, 4:5])
    lo = np.where(tri, np.minimum(v0, np.minimum(v0 + e1, v0 + e2)), v0 - r)
    hi = np.where(tri, np.maximum(v0, np.maximum(v0 + e1, v0 + e2)), v0 + r)
    return lo, hi


class _Report:
    def __init__(self):
        self.items, self.count = [], {}

    def add(self, rule, msg):
        self.count[rule] = self.count.get(rule, 0) + 1
        if self.count[rule] <= MAX_REPORT:
            self.items.append(f"{rule}: {msg}")

    def done(self):
        return self.items + [f"{r}: ... {c} violations in all" for r, c in self.count.items() if c > MAX_REPORT]


def _partition(rep, cover, n):
    miss, dup = np.flatnonzero(cover[:n] == 0), np.flatnonzero(cover[:n] > 1)
    for i in miss[:MAX_REPORT]:
        rep.add("leaves", f"primitive {i} is in no leaf")
    for i in dup[:MAX_REPORT]:
        rep.add("leaves", f"primitive {i} is in {cover[i]} leaves")


def _leaf(rep, what, r, n, max_leaf, cover):
    """Checks one leaf cursor; returns its (first, count) clipped to [0, n) or None."""
    first, count = decode(r)
    ok = True
    if count > max_leaf:
        rep.add("leaves", f"{what}: leaf of {count} primitives, more than {max_leaf}")
    if first < 0 or first + count > n:
        rep.add("leaves", f"{what}: leaf range [{first}, {first + count}) leaves [0, {n})")
        ok = False
    if not ok:
        return None
    cover[first:first + count] += 1
    return first, count


def recomputed_stack(nodes4):
    """Worst-case traversal stack from the nodes alone: entering a node with k
    used slots leaves at most k - 1 entries beneath the child entered.  Needs
    forward-only references (parents before children)."""
    ref = refs4(nodes4)
    used = ~np.isinf(nodes4[:, 0:24]).reshape(len(nodes4), 6, 4).any(axis=1)
    n4 = len(nodes4)
    enter = np.zeros(n4, np.int64)
    worst = 0
    for i in range(n4):
        below = enter[i] + max(int(used[i].sum()), 1) - 1
        worst = max(worst, int(below))
        for k in range(4):
            r = ref[i, k]
            if used[i, k] and i < r < n4:
                enter[r] = max(enter[r], below)
    return worst


def check_bvh4(nodes4, prims, info, max_leaf, exact_stack=False):
    """The four rules over the 4-wide render tree.  info: Device.read_bvh()'s
    "info".  exact_stack: the reported stack must equal the recomputed one
    (pt_upload_scene_lbvh uploads), else only bound it."""
    rep = _Report()
    n, n4 = len(prims), len(nodes4)
    if n4 != info["n_nodes4"] or n != info["n_prims"] or n4 < 1:
        rep.add("topology", f"sizes: {n4} nodes / {n} primitives read, info says {info['n_nodes4']} / {info['n_prims']}")
        return rep.done()
    ref = refs4(nodes4)
    lo, hi = boxes4(nodes4)
    planes = np.isinf(nodes4[:, 0:24]).reshape(n4, 6, 4) & (nodes4[:, 0:24].reshape(n4, 6, 4) > 0)
    unused = planes.any(axis=1)  # a used box has no plane at +inf
    for i, k in zip(*np.nonzero(unused & ~planes.all(axis=1))):
        rep.add("leaves", f"node {i} slot {k}: unused slot with a finite plane")
    # 1. topology
    nref = np.zeros(n4, np.int64)
    forward = True
    for i in range(n4):
        for k in range(4):
            r = int(ref[i, k])
            if unused[i, k] or r < 0:
                continue
            if not i < r < n4:
                rep.add("topology", f"node {i} slot {k}: reference {r} is not forward (need {i} < r < {n4})")
                forward = False
            if 0 <= r < n4:
                nref[r] += 1
    if nref[0]:
        rep.add("topology", f"the root is referenced {nref[0]} times")
    for i in np.flatnonzero(nref[1:] != 1) + 1:
        rep.add("topology", f"node {i} is referenced {nref[i]} times")
    seen = np.zeros(n4, bool)
    todo = [0]
    while todo:
        i = todo.pop()
        if seen[i]:
            continue
        seen[i] = True
        todo += [int(r) for k, r in enumerate(ref[i]) if not unused[i, k] and 0 <= r < n4 and not seen[r]]
    for i in np.flatnonzero(~seen):
        rep.add("topology", f"node {i} is not reachable from the root")
    # 2. leaves
    cover = np.zeros(n + 1, np.int64)
    leaf = {}
    for i in range(n4):
        for k in range(4):
            if not unused[i, k] and ref[i, k] < 0:
                leaf[(i, k)] = _leaf(rep, f"node {i} slot {k}", ref[i, k], n, max_leaf, cover)
    _partition(rep, cover, n)
    # 3. containment (children have larger indices: one pass from the back)
    if forward:
        plo, phi = prim_extent(prims)
        sub_lo = np.full((n4, 3), np.inf)   # primitives below node i
        sub_hi = np.full((n4, 3), -np.inf)
        own_lo = np.full((n4, 3), np.inf)   # union of node i's used child boxes
        own_hi = np.full((n4, 3), -np.inf)
        for i in range(n4 - 1, -1, -1):
            for k in range(4):
                if unused[i, k]:
                    continue
                r = int(ref[i, k])
                if r < 0:
                    fc = leaf.get((i, k))
                    if fc is None:
                        continue
                    a, b = plo[fc[0]:fc[0] + fc[1]].min(0), phi[fc[0]:fc[0] + fc[1]].max(0)
                    what = f"primitives [{fc[0]}, {fc[0] + fc[1]})"
                else:
                    a, b = sub_lo[r], sub_hi[r]
                    what = f"the primitives below node {r}"
                    if (lo[i, k] > own_lo[r]).any() or (hi[i, k] < own_hi[r]).any():
                        rep.add("containment", f"node {i} slot {k}: box does not contain node {r}'s child boxes")
                if (lo[i, k] > a).any() or (hi[i, k] < b).any():
                    short = max((lo[i, k] - a).max(), (b - hi[i, k]).max())
                    rep.add("containment", f"node {i} slot {k}: box does not contain {what} (short by {short:.3g})")
                sub_lo[i], sub_hi[i] = np.minimum(sub_lo[i], a), np.maximum(sub_hi[i], b)
                own_lo[i], own_hi[i] = np.minimum(own_lo[i], lo[i, k]), np.maximum(own_hi[i], hi[i, k])
        rlo, rhi = np.asarray(info["root_lo"], np.float64), np.asarray(info["root_hi"], np.float64)
        if (rlo > own_lo[0]).any() or (rhi < own_hi[0]).any():
            rep.add("containment", f"root box {rlo} .. {rhi} does not contain the root's child boxes "
                                   f"{own_lo[0]} .. {own_hi[0]}")
        # 4. stack
        need = recomputed_stack(nodes4)
        if info["bvh_stack"] < need:
            rep.add("stack", f"reported stack {info['bvh_stack']} is below the tree's worst case {need}")
        elif exact_stack and info["bvh_stack"] != need:
            rep.add("stack", f"reported stack {info['bvh_stack']} is not the tree's worst case {need}")
    return rep.done()


def leaf_cursors4(nodes4):
    ref = refs4(nodes4)
    used = ~np.isinf(nodes4[:, 0:24]).reshape(len(nodes4), 6, 4).any(axis=1)
    return set(int(r) for r in ref[used & (ref < 0)])


def _walk2(nodes2):
    """Nodes reachable from binary node 0 in pre-order, each once; the (node,
    child) pairs that reference a node a second time or out of range."""
    ref = refs2(nodes2)
    n2 = len(nodes2)
    used = ~np.isinf(nodes2[:, 0:12]).any(axis=1)  # (a single-leaf root has an empty second child)
    order, bad, seen, todo = [], [], set(), [0]
    while todo:
        i = todo.pop()
        seen.add(i)
        order.append(i)
        for c in (1, 0):
            r = int(ref[i, c])
            if c == 1 and not used[i]:
                continue
            if r >= 0:
                if r >= n2 or r in seen or r in todo:
                    bad.append((i, c, r))
                else:
                    todo.append(r)
    return order, bad, used


def check_bvh2(nodes2, nodes4, prims, info, max_leaf):
    """Partition and containment over the binary nodes of a pt_upload_scene_lbvh
    upload (their cursors index the same primitive order), and the same set of
    leaves as the 4-wide tree."""
    rep = _Report()
    n, n2 = len(prims), len(nodes2)
    if n2 != info["n_nodes2"] or (n > 4 and n2 != n - 1) or (n <= 4 and n2 not in (1, n - 1)):
        rep.add("topology", f"{n2} binary nodes for {n} primitives (info says {info['n_nodes2']})")
        return rep.done()
    ref = refs2(nodes2)
    lo, hi = boxes2(nodes2)
    order, bad, used = _walk2(nodes2)
    for i, c, r in bad:
        rep.add("topology", f"binary node {i} child {c}: reference {r} is out of range or reached twice")
    cover = np.zeros(n + 1, np.int64)
    plo, phi = prim_extent(prims)
    sub = {}
    own = {}
    cursors = set()
    for i in reversed(order):
        slo, shi = np.full(3, np.inf), np.full(3, -np.inf)
        olo, ohi = np.full(3, np.inf), np.full(3, -np.inf)
        for c in (0, 1):
            if c == 1 and not used[i]:
                continue
            r = int(ref[i, c])
            if r < 0:
                cursors.add(r)
                fc = _leaf(rep, f"binary node {i} child {c}", r, n, max_leaf, cover)
                if fc is None:
                    continue
                a, b = plo[fc[0]:fc[0] + fc[1]].min(0), phi[fc[0]:fc[0] + fc[1]].max(0)
            elif r in sub:
                a, b = sub[r]
                if (lo[i, c] > own[r][0]).any() or (hi[i, c] < own[r][1]).any():
                    rep.add("containment", f"binary node {i} child {c}: box does not contain node {r}'s child boxes")
            else:
                continue
            if (lo[i, c] > a).any() or (hi[i, c] < b).any():
                rep.add("containment", f"binary node {i} child {c}: box does not contain its primitives")
            slo, shi = np.minimum(slo, a), np.maximum(shi, b)
            olo, ohi = np.minimum(olo, lo[i, c]), np.maximum(ohi, hi[i, c])
        sub[i], own[i] = (slo, shi), (olo, ohi)
    _partition(rep, cover, n)
    c4 = leaf_cursors4(nodes4)
    if cursors != c4:
        rep.add("leaves", f"the binary tree's leaves differ from the 4-wide tree's: only binary "
                          f"{sorted(cursors - c4)[:8]}, only 4-wide {sorted(c4 - cursors)[:8]}")
    return rep.done()


def check_order(prims, norms, prim_map, prims_in, norms_in):
    """prim_map is a permutation and the tree's primitives and normals are the
    caller's, bit for bit, in the mapped order."""
    rep = _Report()
    n = len(prims_in)
    pm = np.arange(n) if prim_map is None else np.asarray(prim_map, np.int64)
    if len(pm) != n or len(prims) != n or not np.array_equal(np.sort(pm), np.arange(n)):
        bad = np.flatnonzero(np.bincount(np.clip(pm, 0, n - 1), minlength=n) != 1)
        rep.add("order", f"prim_map is not a permutation of range({n}): entries {bad[:8]} do not appear exactly once")
        return rep.done()
    u = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
    for i in np.flatnonzero((u(prims) != u(prims_in)[pm]).any(axis=1)):
        rep.add("order", f"primitive {i} is not bit-identical to the caller's primitive {pm[i]}")
    for i in np.flatnonzero((u(norms) != u(norms_in)[pm]).any(axis=1)):
        rep.add("order", f"the normals of primitive {i} are not bit-identical to the caller's {pm[i]}")
    return rep.done()


def canonical(nodes4):
    """The tree with its nodes renumbered in depth-first slot order (uint32
    words, references rewritten): equal for two builds that differ only in the
    order their nodes were allocated."""
    ref = refs4(nodes4)
    used = ~np.isinf(nodes4[:, 0:24]).reshape(len(nodes4), 6, 4).any(axis=1)
    new, order, todo = {}, [], [0]
    while todo:
        i = todo.pop()
        if i in new:
            continue
        new[i] = len(order)
        order.append(i)
        todo += [int(ref[i, k]) for k in (3, 2, 1, 0) if used[i, k] and 0 <= ref[i, k] < len(nodes4)]
    out = np.ascontiguousarray(nodes4[order]).view(np.uint32).copy()
    r = out[:, 24:28].view(np.int32)
    for j, i in enumerate(order):
        for k in range(4):
            if used[i, k] and ref[i, k] >= 0:
                r[j, k] = new.get(int(ref[i, k]), -1)
    return out


def sah_cost(nodes2, prims, ci=1.0, max_leaf=4):
    """Surface-area cost of the binary tree in float64 from its read-back
    boxes, in the builder's units: a node costs its half area (the union of
    its two child boxes), a leaf ci x half area x primitives."""
    ref = refs2(nodes2)
    lo, hi = boxes2(nodes2)
    order, _, used = _walk2(nodes2)

    def area(a, b):
        d = b - a
        return d[0] * d[1] + d[1] * d[2] + d[2] * d[0]

    total = 0.0
    for i in order:
        both = (0, 1) if used[i] else (0,)
        total += area(np.min([lo[i, c] for c in both], 0), np.max([hi[i, c] for c in both], 0))
        for c in both:
            if ref[i, c] < 0:
                total += ci * area(lo[i, c], hi[i, c]) * decode(ref[i, c])[1]
    return total


MARGIN = 1e-4


def brute_force(prims, o, d, max_t):
    """Nearest hit and occlusion of rays (o, d) over every primitive, in
    float64, by the kernel's predicates: a triangle is hit where u, v >= 0,
    u + v <= 1 and t > 0 (Moller-Trumbore); a sphere at its nearer root, or
    its farther one when the nearer is behind the origin; occlusion is a hit
    with 0 < t < max_t, a sphere's taken at its farther root.
    Returns hit (bool), prim, t, occluded (bool) and decided (bool): a ray is
    decided when no rounding of the float kernel can change its answers --
    the nearest hit's barycentrics (or a sphere's discriminant, relative to
    r^2) clear MARGIN, its t is MARGIN (relative) away from the next
    candidate's and from 0, every t that matters for occlusion is MARGIN away
    from max_t, and no primitive within those distances is within MARGIN of
    being hit."""
    p = np.asarray(prims, np.float64)
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    max_t = np.asarray(max_t, np.float64)
    m, n = len(o), len(p)
    tri = is_triangle(np.asarray(prims, np.float32))
    v0, e1, e2 = p[None, :, 0:3], p[None, :, 4:7], p[None, :, 8:11]
    O, D = o[:, None, :], d[:, None, :]
    with np.errstate(all="ignore"):
        pv = np.cross(D, e2)
        det = (e1 * pv).sum(-1)
        tv = O - v0
        u = (tv * pv).sum(-1) / det
        qv = np.cross(tv, e1)
        v = (D * qv).sum(-1) / det
        tt = (e2 * qv).sum(-1) / det
        bmin = np.minimum(np.minimum(u, v), 1.0 - u - v)
        bmin = np.where(np.isfinite(bmin) & np.isfinite(tt), bmin, -np.inf)
        # spheres
        r2 = p[None, :, 5]
        bq = (tv * D).sum(-1)
        lp = tv - D * bq[..., None]
        disc = r2 - (lp * lp).sum(-1)
        sq = np.sqrt(np.maximum(disc, 0.0))
        t1, t2 = -bq - sq, -bq + sq
        smargin = np.where(r2 > 0, disc / r2, -np.inf)
    T = tri[None, :]
    # per (ray, primitive): margin of the hit test (> 0 hit), nearest-query t, occlusion t
    marg = np.where(T, bmin, smargin)
    t_near = np.where(T, tt, np.where(t1 > 0, t1, t2))
    t_occ = np.where(T, tt, t2)
    zero = ~T & (np.abs(t1) <= MARGIN * np.maximum(np.abs(t2), 1e-300))  # origin on a sphere's surface
    hitm = (marg >= 0) & (t_near > 0)
    solid = (marg > MARGIN) & (t_near > 0) & ~zero
    maybe = (marg >= -MARGIN) & (t_near > -MARGIN) & ~solid  # could go either way in float
    tn = np.where(hitm, t_near, np.inf)
    prim = tn.argmin(1)
    rows = np.arange(m)
    t = tn[rows, prim]
    hit = np.isfinite(t)
    second = np.where(rows[:, None] * 0 + np.arange(n)[None, :] == prim[:, None], np.inf, tn).min(1) if n > 1 \
        else np.full(m, np.inf)
    reach = np.where(hit, t * (1 + MARGIN), np.inf)
    decided = np.where(hit, solid[rows, prim] & (second > reach), True)
    decided &= ~(maybe & (t_near <= reach[:, None])).any(1)
    # occlusion
    mt = max_t[:, None]
    occm = (marg >= 0) & (t_occ > 0) & (t_occ < mt)
    occluded = occm.any(1)
    sure = ((marg > MARGIN) & ~zero & (t_occ > 0) & (t_occ < mt * (1 - MARGIN))).any(1)
    doubt = ((marg >= -MARGIN) & (t_occ > -MARGIN) & (t_occ < mt * (1 + MARGIN))).any(1)
    decided &= np.where(occluded, sure, ~doubt)
    return {"hit": hit, "prim": np.where(hit, prim, -1), "t": np.where(hit, t, -1.0), "occluded": occluded,
            "decided": decided}
