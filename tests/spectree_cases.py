"""Draft trees for many streams (include/rwkv_mi355x.h rwkv_spec_verify_trees): the cases of tests/test_spec_trees_cpu.py and
tests/test_spec_trees_gpu.py.  Models, start state and ids are those of specseg_cases; a tree is planted on the greedy continuation g of a segment."""
import spec_cases as sc
import specseg_cases as cs

# the planted tree: node j as (parent node, -1 = the segment's last certain row; the depth of the greedy id it carries; that id made wrong).
# The true path 1 - 5 - 7 lies on second siblings; nodes 2 - 3 are a decoy below the wrong node 0: the right ids of depths 1 and 2 or, with `decoy`,
# node 2 carries the pick of node 0's own row -- CONFIRMED by its parent's pick, under a parent that does not stand.
NODES = [(-1, 0, 1), (-1, 0, 0), (0, 1, 0), (2, 2, 0), (1, 1, 1), (1, 1, 0), (5, 2, 1), (5, 2, 0)]
KINDS = dict(whole=[1, 5, 7], none=[], inner=[1, 5])          # the nodes that stand: all of the path, nothing (the root's pick rejects every child), an inner node
DEPTH = 4                                                      # greedy ids a case needs: those of the path and the one behind it
# segments of a 32-row and of a 64-row pass as (slot, certain ids): 30 rows; 60 rows, where the tree on slot 12 has its root on row 30 and nodes 0 / 1 on
# rows 31 / 32 -- the edges root -> 1 and 0 -> 2 cross the halves of the pass
HEADS = {32: [(5, 1), (0, 3), (9, 2)], 64: [(5, 1), (0, 3), (9, 2), (12, 1), (3, 3), (7, 2)]}


def segment(slot, n_certain, g, kind, decoy=None):
    """((slot, ids, n_draft, parent) of the tree planted on g behind the slot's certain ids, the rows of the segment that stand)"""
    ids = [sc.wrong(g[d]) if w else g[d] for _, d, w in NODES]
    if decoy is not None:
        ids[2] = decoy
    if kind == "none":
        ids[1] = sc.wrong(sc.wrong(g[0]))
    if kind == "inner":
        ids[7] = sc.wrong(sc.wrong(g[2]))
    return (slot, cs.certain(slot, n_certain) + ids, len(ids), [0] * n_certain + [n_certain + p for p, _, _ in NODES]), [n_certain + j for j in KINDS[kind]]


def planted(heads, g, rot, decoys=None):
    """segment i of `heads` with the kind (i + rot) % 3: ([segment], [path])"""
    kinds = list(KINDS)
    built = [segment(slot, nc, gi, kinds[(i + rot) % 3], decoys and decoys[i]) for i, ((slot, nc), gi) in enumerate(zip(heads, g))]
    return [b[0] for b in built], [b[1] for b in built]


# refused calls: (segments (slot, n, n_draft), ids or None (all 5), parent or None (a chain), a pick's keywords or None, the message)
REFUSED = [
    ([(0, 3, 2)], None, [0, 0, 2], None, "parent 2 of row 2 must be in 0..1"),               # a parent not below its own row
    ([(0, 4, 2)], None, [0, 0, 0, 1], None, "parent 0 of row 2 must be in 1..1"),            # a parent below the last certain row
    ([(0, 3, 2)], [5, 6, 6], [0, 0, 0], None, "children of row 0 with the same id 6"),
    ([(0, 40, 32)], None, None, None, "n_draft 32 must be in 0..31"),
    ([(0, 40, 0), (1, 30, 0)], None, None, None, "ONE pass"),
    ([(1, 2, 1), (1, 2, 1)], None, None, None, "named twice"),
    ([(0, 2, 1)], None, None, dict(temp=1.0, top_p=0.9, presence=0.5), "penalties are not verified"),
]


def refused_args(eng, segs, ids, parent):
    """(ids, parents, segment array, count) of a REFUSED entry as the C ABI takes them"""
    import ctypes as C
    T = sum(n for _, n, _ in segs)
    chain = [max(0, r - 1) for _, n, _ in segs for r in range(n)]
    return ((C.c_uint64 * T)(*(ids or [5] * T)), (C.c_uint8 * T)(*(parent or chain)), (eng.SpecSegment * len(segs))(*[eng.SpecSegment(s, n, d, 0) for s, n, d in segs]),
            len(segs))
