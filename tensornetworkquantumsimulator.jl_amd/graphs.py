"""Host-side graph helpers: the NamedGraphs / graph_ops.jl subset the hot path needs
(reference: src/graph_ops.jl:6-18,50-64; NamedGraphs.named_grid; SimpleGraphAlgorithms.edge_color via src/imports.jl:9)."""
from __future__ import annotations

import itertools
from collections import deque
from typing import Dict, Hashable, Iterable, List, Sequence, Tuple

Vertex = Hashable


class NamedGraph:
    """Undirected simple graph with ordered, arbitrarily-named vertices.  Vertex ids handed to the C ABI are the
    positions in `vertices`; edge ids are positions in `edges`."""

    def __init__(self, vertices: Sequence[Vertex], edges: Iterable[Tuple[Vertex, Vertex]] = ()):
        self.vertices: List[Vertex] = list(vertices)
        if len(set(self.vertices)) != len(self.vertices):
            raise ValueError("repeated vertex")
        self.index: Dict[Vertex, int] = {v: i for i, v in enumerate(self.vertices)}
        self.edges: List[Tuple[Vertex, Vertex]] = []
        self._adj: Dict[Vertex, List[Vertex]] = {v: [] for v in self.vertices}
        self._eset = set()
        for (a, b) in edges:
            self.add_edge(a, b)

    def add_edge(self, a: Vertex, b: Vertex):
        if a == b:
            raise ValueError("self loops are not supported")
        if a not in self.index or b not in self.index:
            raise KeyError(f"edge ({a}, {b}) names an unknown vertex")
        key = frozenset((a, b))
        if key in self._eset:
            return
        self._eset.add(key)
        self.edges.append((a, b))
        self._adj[a].append(b)
        self._adj[b].append(a)

    def has_edge(self, a, b) -> bool:
        return frozenset((a, b)) in self._eset

    def neighbors(self, v) -> List[Vertex]:
        """neighbours in ascending vertex position (= leg order of the canonical device layout)"""
        return sorted(self._adj[v], key=self.index.__getitem__)

    def degree(self, v) -> int:
        return len(self._adj[v])

    def nv(self) -> int:
        return len(self.vertices)

    def ne(self) -> int:
        return len(self.edges)

    def is_tree(self) -> bool:
        """no cycles (forest): BP defaults use maxiter = 1, no tolerance (beliefpropagationcache.jl:39,110-117)"""
        parent = list(range(len(self.vertices)))

        def find(x):
            while parent[x] != x:
                parent[x] = parent[parent[x]]
                x = parent[x]
            return x
        for (a, b) in self.edges:
            ra, rb = find(self.index[a]), find(self.index[b])
            if ra == rb:
                return False
            parent[ra] = rb
        return True

    def is_connected(self) -> bool:
        if not self.vertices:
            return True
        seen = {self.vertices[0]}
        dq = deque(seen)
        while dq:
            x = dq.popleft()
            for y in self._adj[x]:
                if y not in seen:
                    seen.add(y)
                    dq.append(y)
        return len(seen) == len(self.vertices)


def named_grid(dims, periodic: bool = False) -> NamedGraph:
    """NamedGraphs.named_grid: 1-based tuple vertices, first coordinate fastest.  Periodic dimensions of length
    <= 2 do not wrap (they would collapse onto existing edges)."""
    if isinstance(dims, int):
        dims = (dims,)
    dims = tuple(int(n) for n in dims)
    verts = [tuple(reversed(t)) for t in itertools.product(*[range(1, n + 1) for n in reversed(dims)])]
    g = NamedGraph(verts)
    for v in verts:
        for ax, n in enumerate(dims):
            if v[ax] < n:
                w = v[:ax] + (v[ax] + 1,) + v[ax + 1:]
                g.add_edge(v, w)
            elif periodic and n > 2:
                w = v[:ax] + (1,) + v[ax + 1:]
                g.add_edge(v, w)
    return g


def named_hexagonal_lattice_graph(nx: int, ny: int) -> NamedGraph:
    """honeycomb lattice of nx x ny hexagons (brick-wall construction)"""
    rows, cols = 2 * nx + 2, ny
    dropped = {(0, rows - 1), (cols, (rows - 1) * (cols % 2))}
    nodes = [(i, j) for i in range(cols + 1) for j in range(rows) if (i, j) not in dropped]
    name = {v: (v[0] + 1, v[1] + 1) for v in nodes}
    g = NamedGraph([name[v] for v in nodes])
    present = set(nodes)
    for (i, j) in nodes:
        if (i, j + 1) in present:
            g.add_edge(name[(i, j)], name[(i, j + 1)])
    for (i, j) in nodes:
        if i < cols and i % 2 == j % 2 and (i + 1, j) in present:
            g.add_edge(name[(i, j)], name[(i + 1, j)])
    # keep the edge order of the generator: all column edges, then all row edges
    return g


def heavy_hexagonal_lattice(nx: int, ny: int) -> NamedGraph:
    """src/graph_ops.jl:6-18 -- every edge of the honeycomb lattice gets a decorating vertex"""
    h = named_hexagonal_lattice_graph(nx, ny)
    ren = {v: (2 * v[0] - 1, 2 * v[1] - 1) for v in h.vertices}
    verts = [ren[v] for v in h.vertices]
    edges = []
    for (a, b) in h.edges:
        a2, b2 = ren[a], ren[b]
        mid = ((a2[0] + b2[0]) / 2, (a2[1] + b2[1]) / 2)
        verts.append(mid)
        edges += [(a2, mid), (mid, b2)]
    return NamedGraph(verts, edges)


def named_comb_tree(dims) -> NamedGraph:
    nx, ny = dims
    verts = [(i, j) for j in range(1, ny + 1) for i in range(1, nx + 1)]
    g = NamedGraph(verts)
    for i in range(1, nx):
        g.add_edge((i, 1), (i + 1, 1))
    for i in range(1, nx + 1):
        for j in range(1, ny):
            g.add_edge((i, j), (i, j + 1))
    return g


def build_graph_from_gates(circuit) -> NamedGraph:
    """src/graph_ops.jl:50-64"""
    verts = []
    for gate in circuit:
        vs = gate[1] if isinstance(gate[1], list) else [gate[1]]
        for v in vs:
            if v not in verts:
                verts.append(v)
    g = NamedGraph(verts)
    for gate in circuit:
        vs = gate[1] if isinstance(gate[1], list) else [gate[1]]
        if len(vs) == 2:
            g.add_edge(vs[0], vs[1])
    if not g.is_connected():
        raise RuntimeError("The circuit graph is not connected, meaning the resulting tensor network will be "
                           "disconnected which we do not support.")
    return g


build_graph_from_circuit = build_graph_from_gates


def _bipartition(g: NamedGraph):
    side = {}
    for root in g.vertices:
        if root in side:
            continue
        side[root] = 0
        dq = deque([root])
        while dq:
            x = dq.popleft()
            for y in g._adj[x]:
                if y not in side:
                    side[y] = 1 - side[x]
                    dq.append(y)
                elif side[y] == side[x]:
                    return None
    return side


def edge_color(g: NamedGraph, k: int | None = None) -> List[List[Tuple[Vertex, Vertex]]]:
    """Proper edge colouring into groups of vertex-disjoint edges (role of SimpleGraphAlgorithms.edge_color(g, k),
    src/truncate.jl:20, examples/2dIsing_dynamics.jl:25).  Bipartite graphs get an optimal max-degree colouring
    (Koenig, alternating-path recolouring); other graphs a greedy one.  Raises if more than k colours are needed."""
    maxdeg = max((g.degree(v) for v in g.vertices), default=0)
    color_at: Dict[Vertex, Dict[int, Vertex]] = {v: {} for v in g.vertices}    # vertex -> colour -> neighbour
    ecol: Dict[frozenset, int] = {}

    def free(v, limit):
        for c in range(limit):
            if c not in color_at[v]:
                return c
        return None

    if _bipartition(g) is not None:
        for (u, v) in g.edges:
            a, b = free(u, maxdeg), free(v, maxdeg)
            if a != b and a in color_at[v]:
                # flip the a/b alternating path that starts at v with colour a (it cannot reach u in a bipartite graph)
                path = []
                x, c, d = v, a, b
                while c in color_at[x]:
                    y = color_at[x][c]
                    path.append((x, y, c))
                    x, c, d = y, d, c
                for (x, y, c) in path:
                    del color_at[x][c]
                    del color_at[y][c]
                for (x, y, c) in path:
                    nc = b if c == a else a
                    color_at[x][nc] = y
                    color_at[y][nc] = x
                    ecol[frozenset((x, y))] = nc
            color_at[u][a] = v
            color_at[v][a] = u
            ecol[frozenset((u, v))] = a
    else:
        for (u, v) in g.edges:
            c = 0
            while c in color_at[u] or c in color_at[v]:
                c += 1
            color_at[u][c] = v
            color_at[v][c] = u
            ecol[frozenset((u, v))] = c
    ncol = max(ecol.values(), default=-1) + 1
    if k is not None and ncol > k:
        raise ValueError(f"edge_color: needs {ncol} colours, {k} requested")
    groups: List[List[Tuple[Vertex, Vertex]]] = [[] for _ in range(ncol)]
    for (u, v) in g.edges:
        groups[ecol[frozenset((u, v))]].append((u, v))
    return groups


def forest_cover_edge_sequence(g: NamedGraph) -> List[Tuple[Vertex, Vertex]]:
    """The reference's default BP edge order (beliefpropagationcache.jl:28, NamedGraphs forest_cover_edge_sequence):
    for each spanning forest of a greedy cover, DFS post-order edges towards the root, then their reverses in
    reverse order.  Pass it as `edge_sequence=` to `update` to sweep in the reference's order."""
    remaining = {frozenset(e) for e in g.edges}
    seq: List[Tuple[Vertex, Vertex]] = []
    while remaining:
        visited = set()
        used = set()
        for root in g.vertices:
            if root in visited or not any(frozenset((root, y)) in remaining for y in g._adj[root]):
                continue
            children: Dict[Vertex, List[Vertex]] = {root: []}
            visited.add(root)
            dq = deque([root])
            while dq:
                x = dq.popleft()
                for y in g.neighbors(x):
                    if y not in visited and frozenset((x, y)) in remaining:
                        visited.add(y)
                        children.setdefault(x, []).append(y)
                        children.setdefault(y, [])
                        used.add(frozenset((x, y)))
                        dq.append(y)
            post: List[Tuple[Vertex, Vertex]] = []
            stack = [(root, iter(children[root]))]
            while stack:
                x, it = stack[-1]
                nxt = next(it, None)
                if nxt is None:
                    stack.pop()
                    if stack:
                        post.append((x, stack[-1][0]))
                else:
                    stack.append((nxt, iter(children[nxt])))
            seq.extend(post)
            seq.extend((b, a) for (a, b) in reversed(post))
        remaining -= used
    return seq


def steiner_tree_edges(g: "NamedGraph", verts) -> List[Tuple[Vertex, Vertex]]:
    """Edges of the Steiner tree of the terminals `verts`, as Graphs.steiner_tree builds it (src/expect.jl:67 -> NamedGraphs.steiner_tree ->
    Graphs.jl; [upstream, recalled] -- Kou / Markowsky / Berman): (1) shortest paths from every terminal (unit weights: breadth-first, first in first out, neighbours in
    ascending vertex position; a vertex keeps the FIRST parent that reaches it); (2) minimum spanning tree of the complete graph on the terminals weighted
    by those distances (Kruskal over the pairs (i, j), i < j, in lexicographic order, stable in the weight); (3) every tree pair replaced by its
    shortest path; (4) a minimum spanning tree of the union of those paths (Kruskal over its edges in graph edge order); (5) leaves that are not
    terminals removed until none is left.  Where several shortest paths tie, the choice in (1) decides -- deterministic here, and the same rule
    as the breadth-first search of Graphs.jl, but not pinned against it."""
    terms = list(dict.fromkeys(verts))
    if len(terms) < 2:
        return []
    par, dist = {}, {}
    for t in terms:
        d, p, frontier = {t: 0}, {t: None}, [t]
        while frontier:
            nxt = []
            for a in frontier:
                for b in g.neighbors(a):
                    if b not in d:
                        d[b], p[b] = d[a] + 1, a
                        nxt.append(b)
            frontier = nxt
        par[t], dist[t] = p, d
    for t in terms[1:]:
        if t not in dist[terms[0]]:
            raise ValueError("steiner_tree: the observable's vertices are not connected")

    def kruskal(nodes, wedges):
        comp = {v: v for v in nodes}

        def find(x):
            while comp[x] != x:
                comp[x] = comp[comp[x]]
                x = comp[x]
            return x
        out = []
        for (w, a, b) in sorted(wedges, key=lambda e: e[0]):      # stable: ties keep the enumeration order
            ra, rb = find(a), find(b)
            if ra != rb:
                comp[ra] = rb
                out.append((a, b))
        return out

    closure = [(dist[a][b], a, b) for i, a in enumerate(terms) for b in terms[i + 1:]]
    union = set()
    for (a, b) in kruskal(terms, closure):
        x = b
        while par[a][x] is not None:                               # walk b -> a along a's breadth-first parents
            union.add(frozenset((x, par[a][x])))
            x = par[a][x]
    uverts = sorted({v for e in union for v in e}, key=g.index.__getitem__)
    tree = kruskal(uverts, [(1, a, b) for (a, b) in g.edges if frozenset((a, b)) in union])
    tset = set(terms)
    while True:
        deg = {}
        for (a, b) in tree:
            deg[a] = deg.get(a, 0) + 1
            deg[b] = deg.get(b, 0) + 1
        drop = {v for v, k in deg.items() if k == 1 and v not in tset}
        if not drop:
            return tree
        tree = [(a, b) for (a, b) in tree if a not in drop and b not in drop]


def steiner_region(g: "NamedGraph", verts) -> Tuple[List[Vertex], List[int]]:
    """Vertices of the Steiner tree of `verts` (src/expect.jl:67) as (region, parent): region[0] = verts[0] is the root and parent[i] the index of
    the tree parent of region[i] (-1 for the root).  The library contracts the INDUCED region, like the reference's `norm_factors` over
    `steiner_vs` (src/expect.jl:72): bonds between region vertices that are not tree edges are summed over as well (tnqs_expect_region)."""
    verts = list(verts)
    if len(set(verts)) != len(verts):
        raise ValueError("steiner_region: repeated vertex")
    adj: Dict[Vertex, List[Vertex]] = {}
    for (a, b) in steiner_tree_edges(g, verts):
        adj.setdefault(a, []).append(b)
        adj.setdefault(b, []).append(a)
    region, parent, seen = [verts[0]], [-1], {verts[0]: 0}
    q = 0
    while q < len(region):
        a = region[q]
        for b in sorted(adj.get(a, []), key=g.index.__getitem__):
            if b not in seen:
                seen[b] = len(region); region.append(b); parent.append(q)
        q += 1
    return region, parent


MAX_CONNECTED_CONFIGURATIONS = 200_000      # a guard against an enumeration nobody can wait for, not a tuned number


def connected_edge_components(edges) -> List[Tuple[Tuple[Vertex, Vertex], ...]]:
    """the connected components of the edge-induced subgraph of `edges`, each as a tuple of edges in the order given"""
    comp: Dict[Vertex, Vertex] = {}

    def find(x):
        comp.setdefault(x, x)
        while comp[x] != x:
            comp[x] = comp[comp[x]]
            x = comp[x]
        return x
    for (a, b) in edges:
        comp[find(a)] = find(b)
    out: Dict[Vertex, list] = {}
    for e in edges:
        out.setdefault(find(e[0]), []).append(e)
    return [tuple(c) for c in out.values()]


def leafless_edge_induced_subgraphs(g: NamedGraph, max_edges: int, connected_only: bool = False) -> List[Tuple[Tuple[Vertex, Vertex], ...]]:
    """Role of NamedGraphs.leafless_edge_induced_subgraphs(g, max_edges) in src/MessagePassing/loopcorrection.jl:9: every non-empty set of at most
    `max_edges` edges whose edge-induced subgraph has no vertex of degree 1, as a tuple of edges of `g.edges` in edge order.
    Connected sets are grown inside the 2-core (no edge outside it lies in a leafless subgraph): starting from each edge e, only edges after e are
    added, and only through the exclusive neighbourhood of the set so far, so every connected set is reached exactly once; a branch whose leaves
    cannot all be closed within the budget (one more edge closes at most two) is cut.  What survives are the simple cycles up to `max_edges`, their
    unions, and cycles joined by paths.  Disconnected sets (unless `connected_only`) are the vertex-disjoint unions of connected ones within the budget.
    Order: by number of edges, then by edge positions.  Raises TnqsError when more than MAX_CONNECTED_CONFIGURATIONS connected sets are found."""
    from ._lib import TnqsError
    max_edges = int(max_edges)
    edges = list(g.edges)
    ne = len(edges)
    # 2-core
    alive = [True] * ne
    deg = {v: 0 for v in g.vertices}
    inc: Dict[Vertex, List[int]] = {v: [] for v in g.vertices}
    for i, (a, b) in enumerate(edges):
        deg[a] += 1; deg[b] += 1; inc[a].append(i); inc[b].append(i)
    stack = [v for v in g.vertices if deg[v] == 1]
    while stack:
        v = stack.pop()
        for i in inc[v]:
            if alive[i]:
                alive[i] = False
                for w in edges[i]:
                    deg[w] -= 1
                    if deg[w] == 1:
                        stack.append(w)
    adj = [[] for _ in range(ne)]      # line graph of the 2-core
    for v in g.vertices:
        es = [i for i in inc[v] if alive[i]]
        for i in es:
            adj[i] += [j for j in es if j != i]
    adj = [sorted(set(a)) for a in adj]
    found: List[Tuple[int, ...]] = []
    vdeg: Dict[Vertex, int] = {}

    def add(i, sign):
        for w in edges[i]:
            vdeg[w] = vdeg.get(w, 0) + sign
            if vdeg[w] == 0:
                del vdeg[w]

    def extend(sub, ext, closed, root):
        leaves = sum(1 for d in vdeg.values() if d == 1)
        if leaves == 0:
            found.append(tuple(sorted(sub)))
            if len(found) > MAX_CONNECTED_CONFIGURATIONS:
                raise TnqsError(f"leafless_edge_induced_subgraphs: more than {MAX_CONNECTED_CONFIGURATIONS} connected configurations of at most "
                                f"{max_edges} edges; lower max_configuration_size")
        if len(sub) + max(1, (leaves + 1) // 2) > max_edges:
            return
        ext = list(ext)
        while ext:
            w = ext.pop()
            new = [u for u in adj[w] if u > root and u not in closed]
            sub.append(w); add(w, +1)
            extend(sub, ext + new, closed | set(new), root)
            sub.pop(); add(w, -1)

    if max_edges >= 3:
        for root in range(ne):
            if not alive[root]:
                continue
            nb = [u for u in adj[root] if u > root]
            add(root, +1)
            extend([root], nb, {root} | set(nb), root)
            add(root, -1)
    found.sort(key=lambda c: (len(c), c))
    out = list(found)
    if not connected_only:
        verts = [frozenset(w for i in c for w in edges[i]) for c in found]

        def unions(start, sub, used, size):
            for q in range(start, len(found)):
                c = found[q]
                if size + len(c) > max_edges:
                    break                                # sorted by size: nothing further fits
                if used & verts[q]:
                    continue
                if sub:
                    out.append(tuple(sorted(sub + c)))
                unions(q + 1, sub + c, used | verts[q], size + len(c))
        unions(0, (), frozenset(), 0)
        out = found + sorted(out[len(found):], key=lambda c: (len(c), c))
    return [tuple(edges[i] for i in c) for c in out]
