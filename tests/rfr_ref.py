"""A numpy restatement of the random forest regressor of csrc/rfr.hip, for the tests and for
the fixture generator: the same algorithm in plain integers and float64, not the device code.  No sklearn.

sklearn's RandomForestRegressor(n_estimators, max_depth, min_samples_split, bootstrap=True, max_features=1.0,
random_state=None) behind fit_model's StandardScaler.  The bootstrap is numpy's frozen RandomState stream, drawn
as sklearn draws it; it reaches a tree as integer row weights.  The targets are carried as fixed-point integers
(yq = rint((y - F0) 2^q)), so every weighted sum is an exact int64 and a gain depends on the candidate alone,
and one fixed rule decides among bit-equal gains: the lowest feature index, then the lowest threshold."""
import hashlib
import math

import numpy as np

from tests.gbr_ref import FEATURE_THRESHOLD, Q_MAX, Q_MIN, init_and_q, orders, quantise, standardise32  # noqa: F401

ARRAYS = (("feature", "<i2"), ("threshold", "<f8"), ("left", "<i4"), ("value", "<f8"), ("n_node_samples", "<i4"))


def node_cap(max_depth, n):
    """The padded length of a tree's arrays: a tree of depth d has at most 2^(d+1) - 1 nodes, one on n rows at
    most 2 n - 1."""
    return min((1 << (int(max_depth) + 1)) - 1, 2 * int(n) - 1)


def bootstrap_counts(seed, k, T, n_per_fold):
    """What sklearn's forests draw after np.random.seed(seed): per fold, in fold order, one seed per tree from
    the global stream, then per tree the bincount of n row indices.  A list of k arrays uint8 [T, n_f]."""
    rs = np.random.RandomState(seed)
    out = []
    for f in range(k):
        n = int(n_per_fold[f])
        seeds = rs.randint(np.iinfo(np.int32).max, size=T)
        c = np.stack([np.bincount(np.random.RandomState(s).randint(0, n, n), minlength=n) for s in seeds])
        assert c.max() <= 255
        out.append(c.astype(np.uint8))
    return out


def tree_seeds(seed, k, T):
    """The seeds themselves, [k, T]: sklearn's estimator.random_state."""
    rs = np.random.RandomState(seed)
    return np.stack([rs.randint(np.iinfo(np.int32).max, size=T) for _ in range(k)])


def counts_digest(counts):
    h = hashlib.sha256()
    for c in counts:
        h.update(np.ascontiguousarray(c, dtype="<u1").tobytes())
    return h.hexdigest()


def impurity_leaf(W, S, Q, q):
    """sklearn's impurity <= EPSILON, exactly: W sum w yq^2 - S^2 <= W^2 2^(2q - 52) (python integers)."""
    return W * Q - S * S <= W * W * (1 << (2 * q - 52))


def node_sums(rows, w, yq):
    """(in-bag rows, weighted count, weighted sum, weighted sum of squares) of the rows `rows`, as python ints."""
    ws, ys = [int(v) for v in w[rows]], [int(v) for v in yq[rows]]
    return len(rows), sum(ws), sum(a * b for a, b in zip(ws, ys)), sum(a * b * b for a, b in zip(ws, ys))


def best_of_node(z32_tr, order, mask, w, yq, W, S):
    """The best candidate of the in-bag rows `mask` (at least 2): {feature, threshold, gain, wl, cl, Sl, tied};
    feature -1 when no candidate is valid."""
    D = z32_tr.shape[1]
    cnt = int(mask.sum())
    rec = {"feature": -1, "threshold": 0.0, "gain": -1.0, "wl": 0, "cl": 0, "Sl": 0, "tied": False}
    idx = order[mask[order]].reshape(D, cnt)             # the node's rows in every feature's shared order
    vals = z32_tr[idx, np.arange(D)[:, None]]            # float32 [D, cnt]
    wi = w[idx].astype(np.int64)
    Sl = np.cumsum(wi * yq[idx], axis=1)[:, :-1]         # int64, exact
    wl = np.cumsum(wi, axis=1)[:, :-1]
    wr = W - wl
    a, b = vals[:, :-1], vals[:, 1:]
    valid = b > a + FEATURE_THRESHOLD                    # float32 arithmetic
    diff = wr.astype(np.float64) * Sl.astype(np.float64) - wl.astype(np.float64) * (S - Sl).astype(np.float64)
    gain = diff * diff / (wl.astype(np.float64) * wr.astype(np.float64))
    gain = np.where(valid, gain, -1.0)
    thr = a.astype(np.float64) / 2.0 + b.astype(np.float64) / 2.0
    pos = np.argmax(gain, axis=1)                        # the first maximum: the lowest threshold
    g = gain[np.arange(D), pos]
    j = int(np.argmax(g))                                # the first maximum: the lowest feature
    if g[j] >= 0.0:
        rec.update(feature=j, threshold=float(thr[j, pos[j]]), gain=float(g[j]), wl=int(wl[j, pos[j]]),
                   cl=int(pos[j]) + 1, Sl=int(Sl[j, pos[j]]), tied=bool((g == g[j]).sum() >= 2))
    return rec


def best_split(z32_tr, order, slot, w, yq, nn, q, min_samples_split=2):
    """One level: per node m < nn (slot[p] == m, in-bag rows only) a record {cnt, W, S, feature, threshold, gain,
    wl, cl, Sl, leaf, tied}.  leaf applies sklearn's rules except the depth limit."""
    recs = []
    for m in range(nn):
        mask = (slot == m) & (w > 0)
        cnt, W, S, Q = node_sums(np.nonzero(mask)[0], w, yq)
        rec = {"cnt": cnt, "W": W, "S": S, "feature": -1, "threshold": 0.0, "gain": -1.0, "wl": 0, "cl": 0, "Sl": 0,
               "leaf": True, "tied": False}
        recs.append(rec)
        if cnt < 2:
            continue
        rec.update(best_of_node(z32_tr, order, mask, w, yq, W, S))
        rec["leaf"] = rec["feature"] < 0 or cnt < min_samples_split or impurity_leaf(W, S, Q, q)
    return recs


def build_tree(z32_tr, order, w, yq, init, q, max_depth, min_samples_split, cap):
    """One tree on the rows with w > 0.  Nodes are numbered breadth first: the children of the split nodes of a
    level get consecutive ids in parent order, left then right.  Returns (arrays, node_count, tied, leaf id per
    row, -1 out of bag)."""
    n = len(w)
    w = np.asarray(w, np.int64)
    tree = {"feature": np.full(cap, -1, np.int16), "threshold": np.zeros(cap), "left": np.full(cap, -1, np.int32),
            "value": np.zeros(cap), "n_node_samples": np.zeros(cap, np.int32)}
    node = np.where(w > 0, 0, -1)
    leaf_of = node.copy()
    level_ids, count, tied = [0], 1, 0
    scale = math.ldexp(1.0, -q)
    for level in range(max_depth + 1):
        splits = []
        for i in level_ids:
            mask = node == i
            cnt, W, S, Q = node_sums(np.nonzero(mask)[0], w, yq)
            tree["n_node_samples"][i] = cnt
            tree["value"][i] = init + (float(S) / float(W)) * scale
            leaf_of[mask] = i
            if level == max_depth or cnt < min_samples_split or cnt < 2 or impurity_leaf(W, S, Q, q):
                continue
            rec = best_of_node(z32_tr, order, mask, w, yq, W, S)
            if rec["feature"] >= 0:
                splits.append((i, mask, rec))
        level_ids = []
        for i, mask, rec in splits:
            tree["feature"][i], tree["threshold"][i], tree["left"][i] = rec["feature"], rec["threshold"], count
            tied += int(rec["tied"])
            right = z32_tr[:, rec["feature"]].astype(np.float64) > rec["threshold"]
            assert int((mask & ~right).sum()) == rec["cl"] and int(w[mask & ~right].sum()) == rec["wl"]
            node[mask] = count + right[mask]
            level_ids += [count, count + 1]
            count += 2
        if not level_ids:
            break
    assert count <= cap and n >= 1
    return tree, count, tied, leaf_of


def walk(tree, z32):
    """The id of the leaf each row of z32 reaches."""
    idx = np.zeros(len(z32), np.int64)
    rows = np.arange(len(z32))
    while True:
        fe = tree["feature"][idx].astype(np.int64)
        go = fe >= 0
        if not go.any():
            return idx
        right = z32[rows, np.maximum(fe, 0)].astype(np.float64) > tree["threshold"][idx]
        idx = np.where(go, tree["left"][idx] + right, idx)


def tree_depth(feature, left, node_count):
    """The depth of one tree's deepest node (the root has depth 0)."""
    d = np.zeros(int(node_count), np.int64)
    for i in range(int(node_count)):  # a child's id exceeds its parent's
        if feature[i] >= 0:
            d[left[i]] = d[left[i] + 1] = d[i] + 1
    return int(d.max())


def predict(model, z32):
    """The leaf values summed in tree order in float64, divided by the number of trees."""
    T = len(model["feature"])
    acc = np.zeros(len(z32))
    for t in range(T):
        tree = {key: model[key][t] for key, _ in ARRAYS}
        acc = acc + tree["value"][walk(tree, z32)]
    return acc / float(T)


def fit(z32_tr, y_tr, z32_all, counts, max_depth=20, min_samples_split=100, keep_leaves=False):
    """counts [T, n]: the bootstrap weights.  Returns {feature int16, threshold, left int32, value, n_node_samples
    int32 (all [T, cap]), node_count [T], tied_nodes, init, q, est (all rows of z32_all), leaves [T, n]}."""
    n, D = z32_tr.shape
    T = len(counts)
    y_tr = np.asarray(y_tr, np.float64)
    init, q = init_and_q(y_tr)
    if not Q_MIN <= q <= Q_MAX:
        raise ValueError(f"q = {q}")
    yq, over = quantise(y_tr - init, q, n)
    if over:
        raise OverflowError("targets")
    order = orders(z32_tr)
    cap = node_cap(max_depth, n)
    out = {key: [] for key, _ in ARRAYS}
    node_count, tied_nodes, leaves = np.zeros(T, np.int32), 0, []
    for t in range(T):
        tree, node_count[t], tied, leaf_of = build_tree(z32_tr, order, counts[t], yq, init, q, int(max_depth),
                                                        int(min_samples_split), cap)
        tied_nodes += tied
        for key, _ in ARRAYS:
            out[key].append(tree[key])
        leaves.append(leaf_of)
    out = {key: np.stack(v) for key, v in out.items()}
    out.update(node_count=node_count, tied_nodes=tied_nodes, init=init, q=q,
               leaves=np.stack(leaves) if keep_leaves else None)
    out["est"] = predict(out, z32_all)
    return out


def digest(model):
    h = hashlib.sha256()
    for key, dt in (*ARRAYS, ("node_count", "<i4")):
        h.update(np.ascontiguousarray(model[key], dtype=dt).tobytes())
    return h.hexdigest()
