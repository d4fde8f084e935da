"""An independent statement of include/ngsdist_amd.h "Neighbour-joining trees" in Python floats (IEEE doubles, one rounding
per operation, no contraction): dictionaries keyed by node id, no slots, no prefix -- not a port of the C++.  Also a
generator of additive matrices from random unrooted binary trees whose branch lengths are multiples of 2^-6 (every operation
of the contract is then exact, so neighbour joining must return the tree itself), split extraction from a record, a
Newick reader, and the gap between the best and second-best Q of every step."""
import math
import random

import numpy as np

NAN_BITS = 0x7FF8000000000000


def n_branch(n):
    return 2 * n - 3


def _matrix(v, n):
    d, p = {}, 0
    for a in range(n):
        for b in range(a + 1, n):
            d[a, b] = d[b, a] = float(v[p])
            p += 1
    return d


def nj(v, n, gaps=None):
    """one matrix (n_pairs values in pair order) -> (child list[2n-3], len list[2n-3], status); gaps, a list, receives
    (m, relative gap between the best and the second-best Q) of every join"""
    nb = n_branch(n)
    if not all(math.isfinite(float(x)) for x in v):
        return [-1] * nb, [float("nan")] * nb, 0
    d = _matrix(v, n)
    live = list(range(n))  # ascending node ids: new nodes are appended
    r = {}
    for a in live:
        acc = 0.0
        for b in live:
            if b != a:
                acc += d[a, b]
        r[a] = acc
    child, length = [], []
    m, t = n, 0
    while m > 3:
        best = second = None
        for x in range(m):
            a = live[x]
            for y in range(x + 1, m):
                b = live[y]
                q = (float(m - 2) * d[a, b] - r[a]) - r[b]
                key = (q, a, b)
                if best is None or key < best:
                    best, second = key, best
                elif second is None or key < second:
                    second = key
        if gaps is not None and second is not None:
            gaps.append((m, abs(second[0] - best[0]) / max(abs(best[0]), 5e-324)))
        _, i, j = best
        dij = d[i, j]
        li = 0.5 * dij + (r[i] - r[j]) / (2.0 * float(m - 2))
        child += [i, j]
        length += [li, dij - li]
        u = n + t
        for k in live:
            if k == i or k == j:
                continue
            duk = 0.5 * ((d[i, k] + d[j, k]) - dij)
            r[k] = ((r[k] - d[i, k]) - d[j, k]) + duk
            d[u, k] = d[k, u] = duk
        r[u] = 0.5 * ((r[i] + r[j]) - float(m) * dij)
        live = [k for k in live if k != i and k != j] + [u]
        m -= 1
        t += 1
    a, b, c = live
    child += [a, b, c]
    length += [0.5 * ((d[a, b] + d[a, c]) - d[b, c]), 0.5 * ((d[a, b] + d[b, c]) - d[a, c]), 0.5 * ((d[a, c] + d[b, c]) - d[a, b])]
    return child, length, 1


def nj_many(vals, n, gaps=None):
    """[n_mat][n_pairs] -> (child int32[n_mat][2n-3], len float64, status uint32)"""
    vals = np.asarray(vals, dtype=np.float64).reshape(-1, n * (n - 1) // 2)
    out = [nj(v, n, gaps) for v in vals]
    child = np.array([o[0] for o in out], dtype=np.int32).reshape(len(out), n_branch(n))
    length = np.array([o[1] for o in out], dtype=np.float64).reshape(len(out), n_branch(n))
    length.view(np.uint64)[np.isnan(length)] = NAN_BITS  # a positive quiet NaN, by bits
    return child, length, np.array([o[2] for o in out], dtype=np.uint32)


def _normal(leaves, n):
    s = frozenset(leaves)
    return frozenset(range(n)) - s if 0 in s else s


def record_splits(child, n):
    """the bipartitions of a record's n - 3 joins, in join order, as leaf sets on the side without leaf 0"""
    under = {k: frozenset([k]) for k in range(n)}
    out = []
    for t in range(n - 3):
        under[n + t] = under[int(child[2 * t])] | under[int(child[2 * t + 1])]
        out.append(_normal(under[n + t], n))
    return out


def record_edges(child, length, n):
    """every branch of a record by its bipartition (the leaf set under the entry's node, normalised): {leaf set: length};
    the two m = 4 records of one tree give the same keys"""
    under = {k: frozenset([k]) for k in range(n)}
    for t in range(n - 3):
        under[n + t] = under[int(child[2 * t])] | under[int(child[2 * t + 1])]
    out = {_normal(under[int(c)], n): float(l) for c, l in zip(child, length)}
    assert len(out) == 2 * n - 3
    return out


def random_tree(n, seed):
    """a random unrooted binary tree on the leaves 0 .. n - 1, branch lengths k / 64 with k in 1 .. 64: -> (its additive
    distances in pair order, the set of its internal bipartitions, its 2n - 3 branch lengths sorted)"""
    rng = random.Random(seed)
    step = lambda: rng.randint(1, 64) / 64.0  # noqa: E731
    edges = [(n, 0, step()), (n, 1, step()), (n, 2, step())]
    nxt = n + 1
    for leaf in range(3, n):
        u, v, _ = edges.pop(rng.randrange(len(edges)))
        edges += [(u, nxt, step()), (nxt, v, step()), (nxt, leaf, step())]
        nxt += 1
    adj = {}
    for u, v, l in edges:
        adj.setdefault(u, []).append((v, l))
        adj.setdefault(v, []).append((u, l))
    dist = np.zeros((n, n))
    for a in range(n):
        seen, todo = {a: 0.0}, [a]
        while todo:
            x = todo.pop()
            for y, l in adj[x]:
                if y not in seen:
                    seen[y] = seen[x] + l
                    todo.append(y)
        for b in range(n):
            dist[a, b] = seen[b]
    splits = set()
    for u, v, _ in edges:
        if u < n or v < n:
            continue
        seen, todo = {u}, [u]  # the leaves on u's side of the edge
        while todo:
            x = todo.pop()
            for y, _l in adj[x]:
                if y not in seen and not (x == u and y == v):
                    seen.add(y)
                    todo.append(y)
        splits.add(_normal([x for x in seen if x < n], n))
    iu = np.triu_indices(n, 1)
    return dist[iu], splits, sorted(l for _, _, l in edges)


def parse_newick(text):
    """one Newick line of ngd_nj_newick -> (splits as frozensets of leaf labels under every internal node, in closing
    order; [(name or support text, length text)] of every node in closing order)"""
    text = text.strip()
    assert text.endswith(";")
    pos, stack, splits, nodes = 0, [], [], []
    cur = None
    body = text[:-1]
    while pos < len(body):
        ch = body[pos]
        if ch == "(":
            stack.append([])
            pos += 1
        elif ch == ",":
            pos += 1
        else:
            if ch == ")":
                cur = frozenset().union(*stack.pop())
                pos += 1
                end = pos
                while end < len(body) and body[end] not in ":,()":
                    end += 1
                name = body[pos:end]
                if stack:
                    splits.append(cur)
            else:
                end = pos
                while body[end] != ":":
                    end += 1
                name = body[pos:end]
                cur = frozenset([name])
            pos = end
            ln = ""
            if pos < len(body) and body[pos] == ":":
                end = pos + 1
                while end < len(body) and body[end] not in ",()":
                    end += 1
                ln = body[pos + 1:end]
                pos = end
            if stack:
                stack[-1].append(cur)
                nodes.append((name, ln))
    return splits, nodes
