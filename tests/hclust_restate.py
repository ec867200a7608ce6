"""NumPy restatement of the hclust contract of include/icnv.h (icnv_hclust_dev, DESIGN K9): fastcluster::hclust(as.dist(D),
method) by the nearest-neighbour chain, with the library's operation order and tie rule, rows updated as whole vectors.

  - ward.D2 squares D on entry (d * d) and reports sqrt of each merge dissimilarity.
  - The chain restarts from the first active index when a merge leaves <= 1 element.  Extending it, the tip's nearest
    active neighbour minimises the key (D[tip, j], rank), rank(previous chain element) = -1, else j.
  - x < y merge into y (x retired); Lance-Williams update for every other active k, a = D[x, k], b = D[y, k]:
      single a < b ? a : b   complete a > b ? a : b   average (s*a + t*b) / (s+t)   mcquitty (a + b) * 0.5
      ward   ((v+s)*a - v*c + (v+t)*b) / (s+t+v)
    numpy's elementwise operations round each step and never fuse, so these are the kernel's values bit for bit.
  - r_format: stable sort by dissimilarity, union-find relabelling with R's conventions, left-first order.
"""
import numpy as np

METHODS = {"ward.D": 1, "ward.D2": 2, "single": 3, "complete": 4, "average": 5, "mcquitty": 6, "centroid": 7, "median": 8}


def _lance_williams(code, a, b, c, s, t, v):
    if code == 3:
        return np.where(a < b, a, b)
    if code == 4:
        return np.where(a > b, a, b)
    if code == 5:
        return (s * a + t * b) / (s + t)
    if code == 6:
        return (a + b) * 0.5
    return ((v + s) * a - v * c + (v + t) * b) / (s + t + v)


def nn_chain(dist, method):
    """Raw merges in chain order: (x, y, dissimilarity) with x < y, the dissimilarity squared for ward.D2."""
    code = METHODS[method] if isinstance(method, str) else int(method)
    if code not in (1, 2, 3, 4, 5, 6):
        raise ValueError(f"unsupported method {method!r}")
    D = np.array(dist, dtype=np.float64, copy=True)
    n = D.shape[0]
    if n < 2:
        raise ValueError("must have n >= 2 objects to cluster")
    if code == 2:
        D = D * D
    active = np.ones(n, dtype=bool)
    size = np.ones(n, dtype=np.float64)
    chain, merges, first = [], [], 0
    while len(merges) < n - 1:
        if not chain:
            chain = [first]
        tip = chain[-1]
        prev = chain[-2] if len(chain) > 1 else -1
        cand = active.copy()
        cand[tip] = False
        js = np.flatnonzero(cand)
        vals = D[tip, js]
        o = np.lexsort((np.where(js == prev, -1, js), vals))[0]
        bj, c = int(js[o]), vals[o]
        if bj != prev:
            chain.append(bj)
            continue
        x, y = min(tip, prev), max(tip, prev)
        k = active.copy()
        k[x] = k[y] = False
        nv = _lance_williams(code, D[x, k], D[y, k], c, size[x], size[y], size[k])
        D[y, k] = nv
        D[k, y] = nv
        size[y] = size[x] + size[y]
        active[x] = False
        merges.append((x, y, c))
        while first < n and not active[first]:
            first += 1
        chain = chain[:-2]
        if len(chain) <= 1:
            chain = []
    mx = np.array([m[0] for m in merges], dtype=np.int64)
    my = np.array([m[1] for m in merges], dtype=np.int64)
    mh = np.array([m[2] for m in merges], dtype=np.float64)
    return mx, my, mh


def r_format(n, mx, my, mh, sqrt_heights=False):
    """R's hclust (merge (n-1, 2) int32, height, order int32 1-based) from raw merges in chain order."""
    perm = np.argsort(mh, kind="stable")
    parent = np.arange(2 * n - 1)

    def find(i):
        r = i
        while parent[r] != r:
            r = parent[r]
        while parent[i] != r:
            parent[i], i = r, parent[i]
        return r

    merge = np.zeros((n - 1, 2), dtype=np.int32)
    height = np.zeros(n - 1, dtype=np.float64)
    for i, q in enumerate(perm):
        a, b = sorted((find(int(mx[q])), find(int(my[q]))))
        parent[a] = parent[b] = n + i
        merge[i] = [-(a + 1) if a < n else a - n + 1, -(b + 1) if b < n else b - n + 1]
        height[i] = np.sqrt(mh[q]) if sqrt_heights else mh[q]
    order, stack = [], [n - 1]
    while stack:
        v = stack.pop()
        if v < 0:
            order.append(-v)
        else:
            stack.append(int(merge[v - 1, 1]))
            stack.append(int(merge[v - 1, 0]))
    return merge, height, np.array(order, dtype=np.int32)


def hclust(dist, method="ward.D2"):
    """(merge, height, order) as R's hclust object holds them."""
    n = np.asarray(dist).shape[0]
    mx, my, mh = nn_chain(dist, method)
    return r_format(n, mx, my, mh, sqrt_heights=(method == "ward.D2" or method == 2))


def seq_dist(X):
    """dist(X) (rows = objects) as R's C code computes it: the sequential sum of squared differences, then sqrt."""
    X = np.asarray(X, dtype=np.float64)
    d2 = np.zeros((X.shape[0], X.shape[0]))
    for g in range(X.shape[1]):
        t = X[:, g][:, None] - X[:, g][None, :]
        d2 = d2 + t * t
    return np.sqrt(d2)
