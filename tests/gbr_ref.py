"""A numpy restatement of the gradient boosting regressor of csrc/gbr.hip, for the tests and
for the fixture generator: the same algorithm in plain integers and float64, not the device code.  No sklearn.

sklearn's GradientBoostingRegressor(subsample=1.0, max_features=None, criterion='friedman_mse') behind
fit_model's StandardScaler, with the residual sums carried as fixed-point integers (rq = rint(r 2^q)), so that
every gain is independent of the order of summation, and with one fixed rule among bit-equal gains: the lowest
feature index, then the lowest threshold."""
import hashlib
import math

import numpy as np

FEATURE_THRESHOLD = np.float32(1e-7)  # sklearn/tree/_splitter.pyx, compared in float32
Q_MIN, Q_MAX = 26, 1000


def standardise32(x, mean, scale):
    """(x - mean) / scale with a true float64 division, rounded to float32: what sklearn's trees see."""
    return ((np.asarray(x, np.float64) - mean) / scale).astype(np.float32)


def ceil_log2(n):
    return max(0, (int(n) - 1).bit_length())


def init_and_q(y_tr):
    """F0 = the exactly rounded sum of the targets / n; q = 62 - ceil(log2 n) - e with 2^e > 2 max|y - F0|
    (e minimal; 0 for constant targets)."""
    y_tr = np.asarray(y_tr, np.float64)
    n = len(y_tr)
    init = math.fsum(y_tr.tolist()) / n
    e = math.frexp(2.0 * float(np.max(np.abs(y_tr - init))))[1]
    return init, 62 - ceil_log2(n) - e


def orders(z32_tr):
    """[D, n]: per feature the training positions by value, ties by position."""
    return np.stack([np.argsort(z32_tr[:, j], kind="stable") for j in range(z32_tr.shape[1])]).astype(np.int64)


def quantise(r, q, n):
    rq = np.rint(np.ldexp(np.asarray(r, np.float64), q)).astype(object)
    lim = 1 << (62 - ceil_log2(n))
    over = any(abs(int(v)) >= lim for v in rq)
    return np.array([int(v) if abs(int(v)) < (1 << 63) else 0 for v in rq], dtype=np.int64), over


def impurity_leaf(rq_rows, q):
    """sklearn's impurity <= EPSILON, exactly: n sum rq^2 - S^2 <= n^2 2^(2q - 52)."""
    n = len(rq_rows)
    S = sum(int(v) for v in rq_rows)
    Q = sum(int(v) * int(v) for v in rq_rows)
    return n * Q - S * S <= n * n * (1 << (2 * q - 52))


def best_split(z32_tr, order, node, rq, nn, q):
    """One level: per node m < nn (node[p] == m) a record {cnt, S, feature, threshold, gain, wl, Sl, leaf,
    tied}; feature -1 when no candidate is valid.  leaf applies sklearn's rules except the depth limit."""
    D = z32_tr.shape[1]
    cols = np.arange(D)[:, None]
    recs = []
    for m in range(nn):
        mask = node == m
        cnt = int(mask.sum())
        rec = {"cnt": cnt, "S": 0, "feature": -1, "threshold": 0.0, "gain": -1.0, "wl": 0, "Sl": 0, "leaf": True,
               "tied": False}
        recs.append(rec)
        if cnt == 0:
            continue
        S = int(rq[mask].sum())
        rec["S"] = S
        if cnt < 2:
            continue
        idx = order[mask[order]].reshape(D, cnt)         # the node's rows in every feature's order
        vals = z32_tr[idx, cols]                         # float32 [D, cnt]
        Sl = np.cumsum(rq[idx], axis=1)[:, :-1]          # int64, exact
        wl = np.arange(1, cnt, dtype=np.int64)[None, :]
        wr = cnt - wl
        a, b = vals[:, :-1], vals[:, 1:]
        valid = b > a + FEATURE_THRESHOLD                # float32 arithmetic
        valid &= ~(vals[:, -1:] <= vals[:, :1] + FEATURE_THRESHOLD)  # sklearn's constant-feature rule (implied)
        diff = wr.astype(np.float64) * Sl.astype(np.float64) - wl.astype(np.float64) * (S - Sl).astype(np.float64)
        gain = diff * diff / (wl.astype(np.float64) * wr.astype(np.float64))
        gain = np.where(valid, gain, -1.0)
        thr = a.astype(np.float64) / 2.0 + b.astype(np.float64) / 2.0
        thr = np.where(thr == b.astype(np.float64), a.astype(np.float64), thr)  # sklearn's fallback: never taken
        pos = np.argmax(gain, axis=1)                    # the first maximum: the lowest threshold
        g = gain[np.arange(D), pos]
        j = int(np.argmax(g))                            # the first maximum: the lowest feature
        if g[j] >= 0.0:
            rec.update(feature=j, threshold=float(thr[j, pos[j]]), gain=float(g[j]), wl=int(pos[j]) + 1,
                       Sl=int(Sl[j, pos[j]]), tied=bool((g == g[j]).sum() >= 2))
        rec["leaf"] = rec["feature"] < 0 or impurity_leaf(rq[mask], q)
    return recs


def fit(z32_tr, y_tr, z32_all, learning_rate=0.1, n_estimators=1000, max_depth=3, keep_leaves=False):
    """Returns {feature int16 [T, 2^d - 1], threshold [T, 2^d - 1], value [T, 2^(d+1) - 1], init, q, est (all
    rows of z32_all), train_F, nodes [T], tied_nodes, leaves [T, n] (heap index per training row, on request)}."""
    n, D = z32_tr.shape
    T, depth = int(n_estimators), int(max_depth)
    y_tr = np.asarray(y_tr, np.float64)
    init, q = init_and_q(y_tr)
    if not Q_MIN <= q <= Q_MAX:
        raise ValueError(f"q = {q}")
    order = orders(z32_tr)
    ni, nv = (1 << depth) - 1, (1 << (depth + 1)) - 1
    feature = np.full((T, ni), -1, np.int16)
    threshold, value = np.zeros((T, ni)), np.zeros((T, nv))
    nodes, tied_nodes = np.zeros(T, np.int32), 0
    F_tr, F_all = np.full(n, init), np.full(len(z32_all), init)
    leaves = np.zeros((T, n), np.int32) if keep_leaves else None
    scale = math.ldexp(1.0, -q)
    for s in range(T):
        rq, over = quantise(y_tr - F_tr, q, n)
        if over:
            raise OverflowError(f"stage {s + 1}")
        node = np.zeros(n, np.int64)
        heap = np.zeros(n, np.int64)
        for level in range(depth + 1):
            nn, hb = 1 << level, (1 << level) - 1
            recs = best_split(z32_tr, order, node, rq, nn, q) if level < depth else None
            nxt = np.full(n, -1, np.int64)
            for m in range(nn):
                mask = node == m
                cnt = int(mask.sum())
                if cnt == 0:
                    continue
                value[s, hb + m] = (float(int(rq[mask].sum())) / float(cnt)) * scale
                heap[mask] = hb + m
                if level == depth or recs[m]["leaf"]:
                    continue
                r = recs[m]
                feature[s, hb + m], threshold[s, hb + m] = r["feature"], r["threshold"]
                nodes[s] += 1
                tied_nodes += int(r["tied"])
                right = z32_tr[:, r["feature"]].astype(np.float64) > r["threshold"]
                assert int((mask & ~right).sum()) == r["wl"]
                nxt[mask] = 2 * m + right[mask]
            node = nxt
        if keep_leaves:
            leaves[s] = heap
        F_tr = F_tr + learning_rate * value[s][heap]
        F_all = F_all + learning_rate * value[s][walk(feature[s], threshold[s], z32_all, depth)]
    return {"feature": feature, "threshold": threshold, "value": value, "init": init, "q": q, "est": F_all,
            "train_F": F_tr, "nodes": nodes, "tied_nodes": tied_nodes, "leaves": leaves}


def walk(feature, threshold, z32, depth):
    """Heap index of the leaf each row of z32 reaches in one tree."""
    idx = np.zeros(len(z32), np.int64)
    rows = np.arange(len(z32))
    for _ in range(depth):
        inner = idx < len(feature)
        fe = np.where(inner, feature[np.minimum(idx, len(feature) - 1)], -1)
        go = fe >= 0
        right = z32[rows, np.maximum(fe, 0)].astype(np.float64) > threshold[np.minimum(idx, len(feature) - 1)]
        idx = np.where(go, 2 * idx + 1 + right, idx)
    return idx


def predict(model, z32, learning_rate, depth):
    """init + lr v_1 + lr v_2 + ... in stage order, every product and sum rounded separately."""
    F = np.full(len(z32), float(model["init"]))
    for s in range(len(model["feature"])):
        F = F + learning_rate * model["value"][s][walk(model["feature"][s], model["threshold"][s], z32, depth)]
    return F


def digest(feature, threshold, value):
    h = hashlib.sha256()
    for a, dt in ((feature, "<i2"), (threshold, "<f8"), (value, "<f8")):
        h.update(np.ascontiguousarray(a, dtype=dt).tobytes())
    return h.hexdigest()
