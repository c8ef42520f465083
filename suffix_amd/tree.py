"""`SuffixTree` -- host-side mirror of the reference's suffix tree (suffix_tree/src/lib.rs:46-160) over the
engine's node table (include/suffix_hip.h: sfx_suffix_tree_u32).

    reference (Rust)                          here
    SuffixTree::new(text)             :67     SuffixTree.new(text)
    SuffixTree::from_suffix_table(st) :74     SuffixTree.from_suffix_table(st)
    .text() / .root() / .label(node)  :88     .text() / .root() / .label(node)
    Node::children()                  :109    Node.children()           ordered by first byte
    Node::ancestors()                 :116    Node.ancestors()          self and the root included
    Node::preorder() / leaves()       :123    Node.preorder() / .leaves()
    Node::suffix_indices()            :137    Node.suffix_indices()
    Node::len() / depth()             :142    Node.len() / .depth()
    Node::has_terminals() / suffixes():152    Node.has_terminals() / .suffixes()
    Debug for SuffixTree              :230    repr(tree)

The table is built on the GPU (SA, LCP, node table); the tree itself is never materialised as objects: a `Node`
is a light view -- the dense id of an internal node, or the rank of a leaf and the id of its parent.

The reference's quirks are kept.  A suffix that ends exactly at an internal node is a *terminal* of that node, not a
child of it, so "a node is a leaf iff it has terminals; it may still have children" (:127-131) and leaves() yields such
internal nodes too (:357).  The root carries the empty suffix, index n, as its terminal (SuffixTree::init, :84); its
label is empty, so leaves() skips it.
"""
import ctypes

import numpy as np

from ._lib import default_engine
from .table import SuffixTable, _ptr

_NONE = 0xFFFFFFFF


class Node:
    """A view of one node of a `SuffixTree`: `id` is the dense id of an internal node (None for a leaf), `rank` the
    rank of a leaf (None for an internal node), `parent_id` the dense id of the parent (None for the root)."""
    __slots__ = ("_t", "id", "rank", "parent_id")

    def __init__(self, tree, id, rank, parent_id):
        self._t, self.id, self.rank, self.parent_id = tree, id, rank, parent_id

    def __eq__(self, other):
        return (isinstance(other, Node) and self._t is other._t and self.id == other.id and self.rank == other.rank)

    def __hash__(self):
        return hash((self.id, self.rank))

    def __repr__(self):                                     # Debug for Node (:257-270)
        start, end = self._t._span(self)
        return (f"Node {{ start: {start}, end: {end}, len(children): {self._t._fanout(self)}, "
                f"terminals: {len(self.suffixes())}, parent? {'no' if self.parent_id is None else 'yes'} }}")

    def is_root(self):
        return self.parent_id is None

    def children(self):
        """The children in the order of the first bytes of their labels (a list: len() and reversed() as on the
        reference's ExactSizeIterator + DoubleEndedIterator)."""
        t = self._t
        if self.id is None or not t._n:
            return []
        lo, hi = t._off[self.id], t._off[self.id + 1]
        return [Node(t, c, None, self.id) if c != _NONE else Node(t, None, r, self.id)
                for r, c in zip(t._clb[lo:hi], t._cnode[lo:hi])]

    def ancestors(self):
        """This node, its parent, ... , the root."""
        t, cur = self._t, self
        while True:
            yield cur
            if cur.parent_id is None:
                return
            p = cur.parent_id
            up = t._parent[p]
            cur = Node(t, p, None, None if up == _NONE else up)

    def preorder(self):
        """This node and everything below it, lexicographically (an explicit stack, as :330-342)."""
        t = self._t
        for code, up in t._walk(self):
            yield Node(t, code, None, up) if code >= 0 else Node(t, None, -code - 1, up)

    def leaves(self):
        """Every node at or below this one with a non-empty label and terminals (:357)."""
        return (nd for nd in self.preorder() if nd.len() > 0 and nd.has_terminals())

    def suffix_indices(self):
        """The terminal suffixes of leaves(), in order: from the root, the suffix table."""
        t = self._t
        term, sa = t._term, t._sa
        for code, up in t._walk(self):
            if code < 0:
                yield sa[-code - 1]
            elif up is not None and term[code] != _NONE:      # (the root's label is empty: not a leaf)
                yield term[code]

    def len(self):
        """Bytes of the label into this node."""
        start, end = self._t._span(self)
        return end - start

    __len__ = len

    def depth(self):
        """Number of ancestors, not counting this node."""
        return sum(1 for _ in self.ancestors()) - 1

    def suffixes(self):
        """Terminal suffix indices: the suffix of a leaf, the suffix that ends at an internal node, n at the root."""
        t = self._t
        if self.id is None:
            return [t._sa[self.rank]]
        if self.parent_id is None:
            return [t._n]
        s = t._term[self.id] if t._n else _NONE
        return [] if s == _NONE else [s]

    def has_terminals(self):
        return bool(self.suffixes())

    def suffix_link(self):
        """The node that spells this node's string without its first byte (SuffixTree.suffix_link)."""
        return self._t.suffix_link(self)


class SuffixTree:
    def __init__(self, table, engine=None):
        if not isinstance(table, SuffixTable):
            raise TypeError("SuffixTree is built from a SuffixTable (SuffixTree.new(text) makes one)")
        eng = engine or table._eng
        self._eng = eng
        self._table = table
        self._bytes = table._text
        n = self._n = table.len()
        sa = np.ascontiguousarray(table.table(), dtype=np.uint32)
        arrays = {}
        if n:
            eng.require_device()
            lcp = np.ascontiguousarray(table.lcp_lens(), dtype=np.uint32)
            text = table._tarr
            m, c = ctypes.c_uint64(0), ctypes.c_uint64(0)
            eng.check(eng.lib.sfx_suffix_tree_u32(None, _ptr(sa), _ptr(lcp), n, 0, 0, None, None, None, None, None, None, None, None,
                                                  None, None, ctypes.byref(m), ctypes.byref(c)), "sfx_suffix_tree_u32")
            nm, nc = int(m.value), int(c.value)
            for k in ("node_lb", "node_rb", "node_depth", "node_parent", "node_terminal"):
                arrays[k] = np.zeros(nm, dtype=np.uint32)
            arrays["child_off"] = np.zeros(nm + 1, dtype=np.uint64)
            arrays["child_lb"] = np.zeros(max(nc, 1), dtype=np.uint32)
            arrays["child_node"] = np.zeros(max(nc, 1), dtype=np.uint32)
            arrays["child_byte"] = np.zeros(max(nc, 1), dtype=np.uint8)
            eng.check(eng.lib.sfx_suffix_tree_u32(_ptr(text), _ptr(sa), _ptr(lcp), n, nm, nc, _ptr(arrays["node_lb"]),
                                                  _ptr(arrays["node_rb"]), _ptr(arrays["node_depth"]), _ptr(arrays["node_parent"]),
                                                  _ptr(arrays["node_terminal"]), _ptr(arrays["child_off"]), _ptr(arrays["child_lb"]),
                                                  _ptr(arrays["child_node"]), _ptr(arrays["child_byte"]), None, ctypes.byref(m),
                                                  ctypes.byref(c)), "sfx_suffix_tree_u32")
            for k in ("child_lb", "child_node", "child_byte"):
                arrays[k] = arrays[k][:nc]
        self.arrays = arrays                                      # the node table as numpy arrays (include/suffix_hip.h)
        self._by = None                                           # (lb, rb, depth) -> dense id, made by the first lookup
        # plain lists for the traversals (Python ints: no numpy scalar per step)
        self._sa = sa.tolist()
        self._depth = arrays["node_depth"].tolist() if n else []
        self._parent = arrays["node_parent"].tolist() if n else []
        self._term = arrays["node_terminal"].tolist() if n else []
        self._lb = arrays["node_lb"].tolist() if n else []
        self._off = arrays["child_off"].tolist() if n else [0]
        self._clb = arrays["child_lb"].tolist() if n else []
        self._cnode = arrays["child_node"].tolist() if n else []

    # -- constructors -----------------------------------------------------------------
    @classmethod
    def new(cls, text, engine=None):
        return cls(SuffixTable(text, engine=engine), engine=engine)

    @classmethod
    def from_suffix_table(cls, table, engine=None):
        return cls(table, engine=engine)

    # -- accessors ----------------------------------------------------------------------
    def text(self):
        return self._table.text()

    def root(self):
        return Node(self, 0, None, None)

    def label(self, node):
        """The bytes of the edge into `node` (empty for the root)."""
        start, end = self._span(node)
        return self._bytes[start:end]

    def _span(self, node):
        """[start, end) of the label into the node, as text positions."""
        if node.parent_id is None:
            return 0, 0
        up = self._depth[node.parent_id]
        if node.id is None:
            return self._sa[node.rank] + up, self._n
        s = self._sa[self._lb[node.id]]
        return s + up, s + self._depth[node.id]

    # -- navigation (include/suffix_hip.h: sfx_lce_substr, sfx_lce_lca, sfx_suffix_links_u32) -----------
    def _node(self, k):
        """The view of internal node k."""
        up = self._parent[k] if self._n else _NONE
        return Node(self, k, None, None if up == _NONE else up)

    def _by_interval(self, lb, rb, depth):
        """The internal node (lb, rb, depth): an interval alone does not name a node (the root of a unary text)."""
        if depth == 0:
            return self.root()
        if self._by is None:
            a = self.arrays
            self._by = {key: k for k, key in enumerate(zip(a["node_lb"].tolist(), a["node_rb"].tolist(), self._depth))}
        return self._node(self._by[(lb, rb, depth)])

    def _leaf(self, rank):
        """The leaf of a rank under its parent; leaf_parent is asked of the table call on first use."""
        if "leaf_parent" not in self.arrays:
            eng, n, a = self._eng, self._n, self.arrays
            nm, nc = len(self._depth), len(self._clb)
            lcp = np.ascontiguousarray(self._table.lcp_lens(), dtype=np.uint32)
            sa = np.ascontiguousarray(self._table.table(), dtype=np.uint32)
            tmp = {k: np.zeros_like(a[k]) for k in ("node_lb", "node_rb", "node_depth", "node_parent", "node_terminal", "child_off")}
            clb, cnode = np.zeros(max(nc, 1), dtype=np.uint32), np.zeros(max(nc, 1), dtype=np.uint32)
            leaf_parent = np.zeros(n, dtype=np.uint32)
            m, c = ctypes.c_uint64(0), ctypes.c_uint64(0)
            eng.check(eng.lib.sfx_suffix_tree_u32(None, _ptr(sa), _ptr(lcp), n, nm, nc, _ptr(tmp["node_lb"]), _ptr(tmp["node_rb"]),
                                                  _ptr(tmp["node_depth"]), _ptr(tmp["node_parent"]), _ptr(tmp["node_terminal"]),
                                                  _ptr(tmp["child_off"]), _ptr(clb), _ptr(cnode), None, _ptr(leaf_parent), ctypes.byref(m),
                                                  ctypes.byref(c)), "sfx_suffix_tree_u32")
            a["leaf_parent"] = leaf_parent
        return Node(self, None, int(rank), int(self.arrays["leaf_parent"][rank]))

    def suffix_link(self, node):
        """The node that spells `node`'s string without its first byte; None for the root.  Computed for all internal
        nodes on first use (sfx_suffix_links_u32) and kept as arrays["suffix_link"].  A leaf raises ValueError."""
        if node.id is None:
            raise ValueError("suffix links are kept for internal nodes only")
        if node.parent_id is None:
            return None
        if "suffix_link" not in self.arrays:
            a, nm = self.arrays, len(self._depth)
            sa = np.ascontiguousarray(self._table.table(), dtype=np.uint32)
            lcp = np.ascontiguousarray(self._table.lcp_lens(), dtype=np.uint32)
            out = np.zeros(nm, dtype=np.uint32)
            self._eng.check(self._eng.lib.sfx_suffix_links_u32(_ptr(sa), _ptr(lcp), self._n, nm, _ptr(a["node_lb"]), _ptr(a["node_rb"]),
                                                               _ptr(a["node_depth"]), _ptr(out)), "sfx_suffix_links_u32")
            a["suffix_link"] = out
        return self._node(int(self.arrays["suffix_link"][node.id]))

    def _ranks(self, node):
        if node.id is None:
            return node.rank, node.rank
        return (self._lb[node.id], int(self.arrays["node_rb"][node.id])) if self._n else (0, 0)

    def lca(self, a, b):
        """The lowest common ancestor of two nodes of this tree (either may be a leaf; a node is its own ancestor): the
        LCA of the suffixes at the smallest and the largest rank below them (SuffixTable.lca)."""
        for nd in (a, b):
            if not isinstance(nd, Node) or nd._t is not self:
                raise ValueError("lca takes two nodes of this tree")
        if a == b:
            return a
        if a.parent_id is None or b.parent_id is None:
            return self.root()
        (alo, ahi), (blo, bhi) = self._ranks(a), self._ranks(b)
        lo, hi = min(alo, blo), max(ahi, bhi)
        l, h, d = self._table.lca(self._sa[lo], self._sa[hi])
        return self._by_interval(l, h - 1, d)

    def locus(self, pos, length):
        """The node at or below the locus of text[pos : pos + length]: the highest node whose string starts with it.
        Raises IndexError for a substring that is not inside the text."""
        lo, hi, d = self._table.substring_intervals_batch([int(pos)], [int(length)])
        lo, hi, d = int(lo[0]), int(hi[0]), int(d[0])
        if lo == _NONE:
            raise IndexError(f"text[{int(pos)}:{int(pos) + int(length)}] is not inside the text")
        if int(length) == 0:
            return self.root()
        if hi - lo == 1:                                          # (never a terminal: a terminal's string has two occurrences)
            return self._leaf(lo)
        return self._by_interval(lo, hi - 1, d)

    def _fanout(self, node):
        if node.id is None or not self._n:
            return 0
        return self._off[node.id + 1] - self._off[node.id]

    def _walk(self, node):
        """Preorder below `node` as (code, parent id) pairs: code = the dense id of an internal node, -(rank + 1) for a leaf."""
        if node.id is None:
            yield -node.rank - 1, node.parent_id
            return
        if not self._n:
            yield 0, None
            return
        off, clb, cnode = self._off, self._clb, self._cnode
        stack = [(node.id, node.parent_id)]
        while stack:
            item = stack.pop()
            yield item
            k = item[0]
            if k >= 0:
                for j in range(off[k + 1] - 1, off[k] - 1, -1):          # (reversed: the first child is popped first)
                    c = cnode[j]
                    stack.append((c if c != _NONE else -clb[j] - 1, k))

    def __repr__(self):                                      # Debug for SuffixTree (:230-255)
        out = ["", "-----------------------------------------", "SUFFIX TREE", f"text: {self._bytes.decode('utf-8', 'replace')}"]
        level = {None: -1}
        for nd in self.root().preorder():
            d = level[nd.parent_id] + 1
            if nd.id is not None:
                level[nd.id] = d
            out.append("ROOT" if nd.parent_id is None else " " * (2 * d) + "[" + ", ".join(str(b) for b in self.label(nd)) + "]")
        out.append("-----------------------------------------")
        return "\n".join(out) + "\n"
