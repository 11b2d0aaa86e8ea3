"""The LBVH build restated in numpy from the comments of csrc/dxv_types.h, dxv_math.h and lbvh.hip: no product header, no product
code.  What it states:

  positions   p' = (p - c) / w in float32, (c, w) = centre and half of the largest extent of the box of ALL vertices
  boxes       per triangle min / max of the three p', -+ 2^-16, in float32
  keys        code << 32 | index; the code interleaves the 10-bit cells of the box centre, x above y above z; a cell is
              trunc((centre * 0.5 + 0.5) * 1024) held to [0, 1023]; the keys are sorted as 64-bit numbers
  tree        the binary radix tree over the sorted keys, top down: a range splits behind the last key that agrees with the range's
              first key in the highest bit in which the first and the last key differ; the left part is node g (or leaf ~g when it is
              one key), the right part node g + 1 (or leaf ~(g + 1)), the root is node 0
  parents     (parent << 1) | side for nodes 0 .. T-2 and then leaves 0 .. T-1; the root's word is 0xffffffff
  node boxes  both child boxes of a node: min / max over the child's run of leaves
  heights     a leaf has height 0, a node one more than its higher child; the tree's height is the root's
  tri_extent  over every sampleStride-th workgroup of 256 consecutive triangle indices (stride = workgroups // 256 above 256
              workgroups): sum of uint64(float32((hi_y - lo_y) + (hi_z - lo_z)) * 2^20), then float32(sum / 2^20 / 2 / count)

A node is sixteen 32-bit words: child 0's lo.xyz hi.xyz, child 1's, the two links, the two heights."""
import numpy as np

PAD = np.float32(2.0 ** -16)


def bound_of(vb):
    p = np.asarray(vb, np.float32)[:, :3]
    lo, hi = p.min(0), p.max(0)
    c = (hi + lo) / np.float32(2)
    w = (hi - lo).max() / np.float32(2)
    return np.array([c[0], c[1], c[2], w], np.float32)


def normalised(vb, bound):
    p = np.asarray(vb, np.float32)[:, :3]
    b = np.asarray(bound, np.float32)
    return ((p - b[None, :3]) / b[3]).astype(np.float32)


def tri_boxes(pos, ib):
    """(lo, hi), each (T, 3) float32, in triangle-index order"""
    t = pos[np.asarray(ib).reshape(-1, 3)]
    return (t.min(1) - PAD).astype(np.float32), (t.max(1) + PAD).astype(np.float32)


def cells(lo, hi):
    """(T, 3) 10-bit cells of the box centres"""
    centre = ((lo + hi) * np.float32(0.5)).astype(np.float32)
    u = ((centre * np.float32(0.5) + np.float32(0.5)) * np.float32(1024)).astype(np.float32)
    u = np.where(u > 0, u, np.float32(0))
    u = np.where(u > 1023, np.float32(1023), u)
    return u.astype(np.uint32)


def codes(q):
    code = np.zeros(len(q), np.uint64)
    for bit in range(10):
        for axis, shift in ((0, 2), (1, 1), (2, 0)):
            code |= ((q[:, axis].astype(np.uint64) >> np.uint64(bit)) & np.uint64(1)) << np.uint64(3 * bit + shift)
    return code


def sorted_keys(lo, hi):
    keys = (codes(cells(lo, hi)) << np.uint64(32)) | np.arange(len(lo), dtype=np.uint64)
    return np.sort(keys)


def radix_tree(keys):
    """links (T-1, 2) int32, child heights (T-1, 2) uint32, ranges (T-1, 2) of each node's leaves, split (T-1,), root height.  T >= 2."""
    T = len(keys)
    links = np.zeros((T - 1, 2), np.int64)
    ranges = np.zeros((T - 1, 2), np.int64)
    split = np.zeros(T - 1, np.int64)
    order = []
    kl = [int(k) for k in keys]
    stack = [(0, 0, T - 1)]
    while stack:
        node, lo, hi = stack.pop()
        order.append(node)
        first, last = kl[lo], kl[hi]
        top = (first ^ last).bit_length() - 1                        # the highest bit in which the range's ends differ
        want = ((first >> top) | 1) << top                           # the first number with first's prefix and that bit set
        g = lo + int(np.searchsorted(keys[lo:hi + 1], np.uint64(want), side="left")) - 1
        ranges[node] = (lo, hi)
        split[node] = g
        if g == lo:
            links[node, 0] = ~g
        else:
            links[node, 0] = g
            stack.append((g, lo, g))
        if g + 1 == hi:
            links[node, 1] = ~(g + 1)
        else:
            links[node, 1] = g + 1
            stack.append((g + 1, g + 1, hi))
    heights = np.zeros((T - 1, 2), np.int64)
    total = np.zeros(T - 1, np.int64)
    for node in reversed(order):
        for side in (0, 1):
            c = links[node, side]
            heights[node, side] = 0 if c < 0 else total[c]
        total[node] = heights[node].max() + 1
    assert len(order) == T - 1
    return links.astype(np.int32), heights.astype(np.uint32), ranges, split, int(total[0])


def parent_words(links):
    T = len(links) + 1
    out = np.zeros(2 * T - 1, np.uint32)
    for side in (0, 1):
        c = links[:, side].astype(np.int64)
        slot = np.where(c >= 0, c, (T - 1) + ~c)
        out[slot] = (np.arange(T - 1, dtype=np.uint32) << np.uint32(1)) | np.uint32(side)
    out[0] = 0xffffffff
    return out


def _range_reduce(fn, values, lo, hi):
    """fn-reduction of values[lo[i] .. hi[i]] (inclusive) for every i"""
    idx = np.empty(2 * len(lo), np.int64)
    idx[0::2] = lo
    idx[1::2] = hi + 1
    padded = np.concatenate([values, values[-1:]])                   # (reduceat wants every index inside the array)
    return fn.reduceat(padded, idx, axis=0)[0::2]


def node_words(links, heights, ranges, split, lo_sorted, hi_sorted):
    """the (T-1, 16) uint32 words of the nodes from the leaf boxes in Morton order"""
    n = len(links)
    out = np.zeros((n, 16), np.uint32)
    f = out.view(np.float32)
    f[:, 0:3] = _range_reduce(np.minimum, lo_sorted, ranges[:, 0], split)
    f[:, 3:6] = _range_reduce(np.maximum, hi_sorted, ranges[:, 0], split)
    f[:, 6:9] = _range_reduce(np.minimum, lo_sorted, split + 1, ranges[:, 1])
    f[:, 9:12] = _range_reduce(np.maximum, hi_sorted, split + 1, ranges[:, 1])
    out[:, 12:14] = links.view(np.uint32)
    out[:, 14:16] = heights
    return out


def tri_extent(lo, hi):
    T = len(lo)
    groups = (T + 255) // 256
    stride = groups // 256 if groups > 256 else 1
    ext = ((hi[:, 1] - lo[:, 1]).astype(np.float32) + (hi[:, 2] - lo[:, 2]).astype(np.float32)).astype(np.float32)
    fixed = (ext * np.float32(1048576.0)).astype(np.float32).astype(np.uint64)
    total, count = 0, 0
    for g in range(0, groups, stride):
        total += int(fixed[256 * g:256 * (g + 1)].sum(dtype=np.uint64))
        count += min(256, T - 256 * g)
    return np.float32(float(total) / 1048576.0 / 2.0 / float(count))


class Build:
    """everything above for one mesh; bound: the build's (c, w), default the mesh's own; tree=False: keys and figures only"""

    def __init__(self, vb, ib, bound=None, tree=True):
        self.ib = np.asarray(ib, np.uint32)
        self.T = len(self.ib) // 3
        self.bound = bound_of(vb) if bound is None else np.asarray(bound, np.float32)
        self.pos = normalised(vb, self.bound)
        self.lo, self.hi = tri_boxes(self.pos, self.ib)
        self.keys = sorted_keys(self.lo, self.hi)
        self.order = (self.keys & np.uint64(0xffffffff)).astype(np.int64)        # triangle index of every Morton slot
        self.tri_extent = tri_extent(self.lo, self.hi)
        self.root_lo, self.root_hi = self.lo.min(0), self.hi.max(0)
        self.has_tree = bool(tree) and self.T > 1
        if self.has_tree:
            self.links, self.heights, self.ranges, self.split, self.height = radix_tree(self.keys)
            self.parents = parent_words(self.links)
            self.nodes = node_words(self.links, self.heights, self.ranges, self.split, self.lo[self.order], self.hi[self.order])
        elif self.T == 1:
            self.height = 1                                                       # (one node; its second child is a dummy: not restated)

    def tri_pos(self):
        """(T, 3, 3): the three normalised positions of every Morton slot"""
        return self.pos[self.ib.reshape(-1, 3)[self.order]]

    def refit(self, vb):
        """the node words after the vertices moved: same links, same heights, boxes of the new positions in the old order"""
        lo, hi = tri_boxes(normalised(vb, self.bound), self.ib)
        return node_words(self.links, self.heights, self.ranges, self.split, lo[self.order], hi[self.order]), lo.min(0), hi.max(0)


# ---- the half-float copies: properties, on a download -------------------------------------------------------------------
def half_planes(words32):
    """(n, 12) float64 decoded planes of (n, 8) uint32 compressed nodes: [axis * 4 + {lo0, lo1, hi0, hi1}]"""
    return np.ascontiguousarray(words32).view(np.uint16).reshape(len(words32), 16)[:, :12].view(np.float16).astype(np.float64)


def outward_violations(nodes, words32):
    """rows of the compressed copy with a plane that is not the tightest outward half float of the exact plane"""
    exact = np.ascontiguousarray(nodes[:, :12]).view(np.float32).astype(np.float64)
    h = np.ascontiguousarray(words32).view(np.uint16).reshape(len(words32), 16)[:, :12].view(np.float16)
    bad = np.zeros(len(nodes), bool)
    with np.errstate(over="ignore"):
        for axis in range(3):
            for child in (0, 1):
                lo_exact, hi_exact = exact[:, 6 * child + axis], exact[:, 6 * child + 3 + axis]
                lo, hi = h[:, axis * 4 + child], h[:, axis * 4 + 2 + child]
                lo_in = np.nextafter(lo, np.float16(np.inf)).astype(np.float64)
                hi_in = np.nextafter(hi, np.float16(-np.inf)).astype(np.float64)
                lo, hi = lo.astype(np.float64), hi.astype(np.float64)
                bad |= ~((lo <= lo_exact) & ((lo == lo_exact) | (lo_in > lo_exact)))
                bad |= ~((hi >= hi_exact) & ((hi == hi_exact) | (hi_in < hi_exact)))
    return np.flatnonzero(bad)


NO_CHILD = np.int32(-0x80000000)


def wide_from_32(words32):
    """the (n, 16) uint32 wide nodes dxv_types.h describes, arranged from the compressed ones: every internal child replaced by its two
    children, in order; b[axis * 8 + side * 4 + slot]; unused slots [+inf, -inf] and kNoChild"""
    n = len(words32)
    h = np.ascontiguousarray(words32).view(np.uint16).reshape(n, 16)
    link = np.ascontiguousarray(words32)[:, 6:8].view(np.int32)
    out = np.zeros((n, 32), np.uint16)
    out[:, [a * 8 + s for a in range(3) for s in range(4)]] = 0x7c00
    out[:, [a * 8 + 4 + s for a in range(3) for s in range(4)]] = 0xfc00
    c = np.full((n, 4), NO_CHILD, np.int32)
    slot = np.zeros(n, np.int64)
    rows = np.arange(n)

    def emit(mask, src, child, lnk):
        r = rows[mask]
        for a in range(3):
            out[r, a * 8 + slot[mask]] = h[src, a * 4 + child]
            out[r, a * 8 + 4 + slot[mask]] = h[src, a * 4 + 2 + child]
        c[r, slot[mask]] = lnk
        slot[mask] += 1

    for side in (0, 1):
        inner = link[:, side] >= 0
        m = link[inner, side]
        emit(inner, m, 0, link[m, 0])
        emit(inner, m, 1, link[m, 1])
        leaf = ~inner
        emit(leaf, rows[leaf], side, link[leaf, side])
    out32 = out.view(np.uint32).reshape(n, 16).copy()
    out32[:, 12:16] = c.view(np.uint32)
    return out32
