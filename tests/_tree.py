"""Shared pieces of the suffix-tree node-table tests (test_tree_emu.py, test_gpu_tree.py). TEST INFRASTRUCTURE ONLY.

 - `reference_tree`: a Python restatement of the reference's `to_suffix_tree` (suffix_tree/src/lib.rs:392-505), written
   from reading it: `ancestor_lcp_len` (:393-410), the `Equal` branch that hangs a new leaf under `vins` (:421-441) and
   the `Less` branch that cuts the right-most edge, makes an internal node and re-parents the right-most child under it
   (:442-500).  `canonical` turns it into nested tuples (path length, label bytes, terminals, children by key).
 - `canonical_from_arrays`: the engine's ten arrays as the same nested tuples.
 - `tree_u32` / `tree_dev`: the two entry points of include/suffix_hip.h on numpy arrays.
 - `build_checker` / `check_arrays`: tests/tree_check.c, the serial stack sweep that writes all ten arrays.
"""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
NONE = 0xFFFFFFFF
OK, ERR_ARG, ERR_TOO_LARGE, ERR_WORKSPACE = 0, 1, 2, 5
NODE_ARRAYS = ("node_lb", "node_rb", "node_depth", "node_parent", "node_terminal")
ALL_ARRAYS = NODE_ARRAYS + ("child_off", "child_lb", "child_node", "child_byte", "leaf_parent")
DTYPES = {**{k: np.uint32 for k in ALL_ARRAYS}, "child_off": np.uint64, "child_byte": np.uint8}


# ---- the reference's sweep, restated ---------------------------------------------------------------------------------
class RNode:
    __slots__ = ("parent", "children", "suffixes", "start", "end", "path_len")

    def __init__(self, suffixes, start, end):                # Node::leaf (:163-172) / Node::internal (:174-183)
        self.parent, self.children, self.suffixes = None, {}, suffixes
        self.start, self.end, self.path_len = start, end, 0

    def len(self):
        return self.end - self.start

    def add_parent(self, node):                              # :193-196
        self.parent = node
        self.path_len = node.path_len + self.len()


def reference_tree(text, sa, lcp):
    n = len(text)
    root = RNode([n], 0, 0)                                  # SuffixTree::init (:78-85): the root is a "leaf" of the empty suffix

    def key(node):                                           # :102-104
        return text[node.start]

    def ancestor_lcp_len(cur, lcplen):                       # :393-410
        while cur.path_len > lcplen and cur.parent is not None:
            cur = cur.parent
        return cur

    last = root
    for i in range(n):
        sufstart, lcp_len = int(sa[i]), int(lcp[i])
        vins = ancestor_lcp_len(last, lcp_len)
        dv = vins.path_len
        if dv == lcp_len:                                    # Ordering::Equal (:421-441)
            node = RNode([sufstart], sufstart + lcp_len, n)
            node.add_parent(vins)
            first = key(node)
            assert first not in vins.children
            last = node
            vins.children[first] = node
        else:                                                # Ordering::Less (:442-500)
            assert dv < lcp_len and vins.children
            rkey = max(vins.children)
            rnode = vins.children.pop(rkey)
            prev = int(sa[i - 1])
            int_node = RNode([], prev + dv, prev + lcp_len)
            int_node.add_parent(vins)
            rnode.start = prev + lcp_len
            rnode.end = prev + rnode.path_len
            rnode.add_parent(int_node)
            leaf = RNode([sufstart], sufstart + lcp_len, n)
            leaf.add_parent(int_node)
            last = leaf
            assert key(rnode) != key(leaf)
            int_node.children[key(rnode)] = rnode
            int_node.children[key(leaf)] = leaf
            vins.children[key(int_node)] = int_node
    return root


def canonical(text, root):
    """(path length, label bytes, terminals, ((key, child), ...) by key) -- built bottom-up without recursion."""
    done = {}
    stack = [(root, False)]
    while stack:
        node, seen = stack.pop()
        if not seen:
            stack.append((node, True))
            stack.extend((c, False) for c in node.children.values())
        else:
            kids = tuple((k, done.pop(id(node.children[k]))) for k in sorted(node.children))
            done[id(node)] = (node.path_len, bytes(text[node.start:node.end]), tuple(node.suffixes), kids)
    return done[id(root)]


def canonical_from_arrays(text, sa, a):
    """The engine's arrays in the same form.  The reference's root carries the empty suffix (index n) as a terminal
    (:84); the table gives the root none, so it is added here."""
    n = len(text)
    if n == 0:
        return (0, b"", (0,), ())
    depth, term, off = a["node_depth"].tolist(), a["node_terminal"].tolist(), a["child_off"].tolist()
    clb, cnode, cbyte = a["child_lb"].tolist(), a["child_node"].tolist(), a["child_byte"].tolist()
    sa = np.asarray(sa).tolist()
    done = {}
    stack = [(0, 0, 0, False)]                               # (node id, first rank, depth of the parent, seen)
    while stack:
        k, lb, up, seen = stack.pop()
        if not seen:
            stack.append((k, lb, up, True))
            stack.extend((cnode[j], clb[j], depth[k], False) for j in range(off[k], off[k + 1]) if cnode[j] != NONE)
            continue
        kids = []
        for j in range(off[k], off[k + 1]):
            if cnode[j] != NONE:
                kids.append((cbyte[j], done.pop(cnode[j])))
            else:
                s = sa[clb[j]]
                kids.append((cbyte[j], (n - s, bytes(text[s + depth[k]:]), (s,), ())))
        terms = (n,) if k == 0 else (() if term[k] == NONE else (term[k],))
        done[k] = (depth[k], bytes(text[sa[lb] + up:sa[lb] + depth[k]]), terms, tuple(kids))
    return done[0]


# ---- the entry points on numpy arrays ----------------------------------------------------------------------------------
def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None else None


def alloc(n, m, c, fill=0xFF, leaf_parent=True, child_byte=True):
    out = {k: np.full(m, fill * 0x01010101, dtype=np.uint32) for k in NODE_ARRAYS}
    out["child_off"] = np.full(m + 1, fill * 0x0101010101010101, dtype=np.uint64)
    out["child_lb"] = np.full(c, fill * 0x01010101, dtype=np.uint32)
    out["child_node"] = np.full(c, fill * 0x01010101, dtype=np.uint32)
    out["child_byte"] = np.full(c, fill, dtype=np.uint8) if child_byte else None
    out["leaf_parent"] = np.full(n, fill * 0x01010101, dtype=np.uint32) if leaf_parent else None
    return out


def call_u32(eng, text, sa, lcp, node_cap, child_cap, out):
    """One sfx_suffix_tree_u32 call -> (status, m, C)."""
    t = np.frombuffer(text, dtype=np.uint8) if text is not None else None
    m, c = ctypes.c_uint64(NONE), ctypes.c_uint64(NONE)
    rc = eng.lib.sfx_suffix_tree_u32(_ptr(t), _ptr(sa), _ptr(lcp), len(sa), node_cap, child_cap, *[_ptr(out.get(k)) for k in ALL_ARRAYS],
                                     ctypes.byref(m), ctypes.byref(c))
    return rc, int(m.value), int(c.value)


def tree_u32(eng, text, sa, lcp):
    """Sizing call + filling call on host arrays -> dict of the ten arrays, cut to m and C."""
    sa, lcp = np.ascontiguousarray(sa, dtype=np.uint32), np.ascontiguousarray(lcp, dtype=np.uint32)
    rc, m, c = call_u32(eng, None, sa, lcp, 0, 0, {})
    assert rc == OK, rc
    out = alloc(len(sa), m, c)
    rc, m2, c2 = call_u32(eng, text, sa, lcp, m, c, out)
    assert rc == OK and (m2, c2) == (m, c), (rc, m, c, m2, c2)
    return out


def build_checker(out_dir):
    """tests/tree_check.c -> an executable."""
    exe = os.path.join(str(out_dir), "tree_check")
    subprocess.check_call(["gcc", "-O2", "-std=c99", "-o", exe, os.path.join(HERE, "tree_check.c")])
    return exe


def check_arrays(exe, out_dir, text, sa, lcp):
    """Runs the checker -> its ten arrays."""
    d = str(out_dir)
    paths = []
    for name, arr in (("text", np.frombuffer(text, dtype=np.uint8)), ("sa", sa), ("lcp", lcp)):
        p = os.path.join(d, name + ".in")
        np.ascontiguousarray(arr).tofile(p)
        paths.append(p)
    line = subprocess.run([exe, *paths, d], check=True, capture_output=True, text=True).stdout.split()
    out = {k: np.fromfile(os.path.join(d, k + ".bin"), dtype=DTYPES[k]) for k in ALL_ARRAYS}
    assert (int(line[0]), int(line[1])) == (out["node_lb"].size, out["child_lb"].size)
    return out


def assert_equal_arrays(got, exp, what=""):
    for k in ALL_ARRAYS:
        assert got[k].dtype == exp[k].dtype and np.array_equal(got[k], exp[k]), (what, k, got[k][:16], exp[k][:16])


def check_invariants(text, sa, a):
    """The count identity, ascending first ranks and first bytes inside every node, leaf_parent against the child lists."""
    n, m, c = len(text), a["node_lb"].size, a["child_lb"].size
    t = int((a["node_terminal"] != NONE).sum())
    assert c == n - 1 + m - t, (n, m, t, c)
    off = a["child_off"].astype(np.int64)
    assert off[0] == 0 and off[m] == c and np.all(np.diff(off) >= 0)
    owner = np.repeat(np.arange(m), np.diff(off))
    inner = np.flatnonzero(owner[1:] == owner[:-1]) + 1                 # entries that have a predecessor in their node
    assert np.all(a["child_lb"][inner] > a["child_lb"][inner - 1])
    assert np.all(a["child_byte"][inner] > a["child_byte"][inner - 1])
    assert np.all(np.diff(off) <= 256)
    exp = np.full(n, NONE, dtype=np.uint32)
    leaves = a["child_node"] == NONE
    exp[a["child_lb"][leaves]] = owner[leaves]
    has = np.flatnonzero(a["node_terminal"] != NONE)
    assert np.all(exp[a["node_lb"][has]] == NONE)                       # (a terminal is nobody's child)
    exp[a["node_lb"][has]] = has
    assert np.array_equal(np.asarray(sa)[a["node_lb"][has]], a["node_terminal"][has])
    assert np.array_equal(a["leaf_parent"], exp)
    kids = np.flatnonzero(~leaves)
    assert np.array_equal(a["node_parent"][a["child_node"][kids]], owner[kids].astype(np.uint32))
    assert np.array_equal(a["node_lb"][a["child_node"][kids]], a["child_lb"][kids])
    assert a["node_parent"][0] == NONE and a["node_lb"][0] == 0 and a["node_rb"][0] == n - 1 and a["node_depth"][0] == 0


FIXED_TEXTS = [b"mississippi", b"apple", b"x", b"a" * 70, b"ab" * 40 + b"a"]


def fixed_texts():
    import random
    fib = [b"b", b"a"]
    while len(fib[-1]) < 300:
        fib.append(fib[-1] + fib[-2])
    rng = random.Random(600)
    every = list(range(256))
    rng.shuffle(every)
    return FIXED_TEXTS + [fib[-1], bytes(every), bytes(rng.randrange(256) for _ in range(600))]


# ---- sfx_suffix_tree_dev on guarded buffers (tests/_buffers.py, as it is) ------------------------------------------------
def dev_case(eng, device, text, sa, lcp, node_cap, child_cap, offsets=False, ws_fill=0xFF, ws_short=0, with_text=True,
             leaf_parent=True, drop=()):
    """One sfx_suffix_tree_dev call with every array between guard bands -> (status, m, C, inputs, outputs incl. workspace).
    offsets: text and every array at offset addresses (child_byte at an odd one); the workspace is exactly
    sfx_suffix_tree_workspace_bytes(n) - ws_short bytes, filled with ws_fill; `drop` names arrays passed as NULL."""
    import _buffers as B
    n = len(sa)
    u32 = (lambda i: B.U32_OFFSETS[i % 3]) if offsets else (lambda i: 0)
    ins = {"sa": B.inp(np.ascontiguousarray(sa, dtype=np.uint32), device, u32(0)),
           "lcp": B.inp(np.ascontiguousarray(lcp, dtype=np.uint32), device, u32(1))}
    if with_text:
        ins["text"] = B.text_in(text, device, 3 if offsets else 0)
    outs = {k: B.guarded(4 * node_cap, device, u32(2 + i), 0xFF) for i, k in enumerate(NODE_ARRAYS)}
    outs["child_off"] = B.guarded(8 * (node_cap + 1), device, 8 if offsets else 0, 0xFF)
    outs["child_lb"] = B.guarded(4 * child_cap, device, u32(1), 0xFF)
    outs["child_node"] = B.guarded(4 * child_cap, device, u32(2), 0xFF)
    outs["child_byte"] = B.guarded(child_cap, device, 5 if offsets else 0, 0xFF)
    outs["leaf_parent"] = B.guarded(4 * n, device, u32(0), 0xFF)
    ws = B.guarded(int(eng.lib.sfx_suffix_tree_workspace_bytes(n)) - ws_short, device, 0, ws_fill)
    m, c = ctypes.c_uint64(NONE), ctypes.c_uint64(NONE)

    def p(k):
        if k in drop or (k == "child_byte" and not with_text) or (k == "leaf_parent" and not leaf_parent):
            return None
        return outs[k].ptr
    rc = eng.lib.sfx_suffix_tree_dev(ins["text"].ptr if with_text and "text" not in drop else None, ins["sa"].ptr, ins["lcp"].ptr, n,
                                     node_cap, child_cap, *[p(k) for k in ALL_ARRAYS], ctypes.byref(m), ctypes.byref(c), ws.ptr,
                                     ws.nbytes, B.stream_of(device))
    outs["workspace"] = ws
    return rc, int(m.value), int(c.value), ins, outs


def dev_arrays(outs, m, c, n):
    """The guarded outputs of dev_case, cut to m and C."""
    cut = {**{k: m for k in NODE_ARRAYS}, "child_off": m + 1, "child_lb": c, "child_node": c, "child_byte": c, "leaf_parent": n}
    return {k: outs[k].host(DTYPES[k])[:cut[k]] for k in ALL_ARRAYS}


def untouched(outs, names=ALL_ARRAYS):
    return all(bool((outs[k].host() == 0xFF).all()) for k in names)
