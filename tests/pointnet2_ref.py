"""Float32 numpy restatement of the pointnet2_batch ops (include/spx.h §11, csrc/pointnet2.hip), written from their
stated semantics.  A helper module for the tests, not a test file.

Every float32 operation here rounds once, exactly like the uncontracted kernels: distances are
((dx*dx) + (dy*dy)) + (dz*dz) with dx = a - b."""
import numpy as np

F32 = np.float32


def sq_dist(a, b):
    """a (..., 3), b broadcastable (..., 3) -> float32 squared distance in the kernels' association."""
    d = (np.asarray(a, F32) - np.asarray(b, F32)).astype(F32)
    return ((d[..., 0] * d[..., 0]) + (d[..., 1] * d[..., 1])) + (d[..., 2] * d[..., 2])


def fps_log2_bs(n):
    """log2 of the reference's FPS block size min(2^floor(log2 n), 1024)."""
    return min(int(n).bit_length() - 1, 10)


def _bitrev(v, bits):
    out = np.zeros_like(v)
    for i in range(bits):
        out |= ((v >> i) & 1) << (bits - 1 - i)
    return out


def fps_priority(n):
    """Tie priority of every point (smaller wins): (bitrev(k mod bs), k div bs)."""
    L = fps_log2_bs(n)
    k = np.arange(n, dtype=np.int64)
    return (_bitrev(k & ((1 << L) - 1), L) << 32) | (k >> L)


def weighted_rank(temp, w):
    """(float)((double)temp * max((double)w, 1e-12))"""
    return (temp.astype(np.float64) * np.maximum(w.astype(np.float64), 1e-12)).astype(F32)


def _pick(v, prio):
    """Arg-max of v (B, N) over the values > -1, ties to the smallest priority; 0 where nothing is > -1."""
    cand = v > F32(-1)
    vm = np.where(cand, v, -np.inf)
    best = vm.max(axis=1, keepdims=True)
    tie = cand & (vm == best)
    p = np.where(tie, prio[None, :], np.iinfo(np.int64).max)
    k = p.argmin(axis=1)
    return np.where(cand.any(axis=1), k, 0)


def furthest_point_sample(npoint, xyz=None, matrix=None, weights=None):
    """xyz (B, N, 3) or matrix (B, N, N); weights (B, N) or None -> (B, npoint) int32.  Vectorised over the batch."""
    src = np.asarray(xyz if matrix is None else matrix, F32)
    B, N = src.shape[:2]
    w = None if weights is None else np.asarray(weights, F32)
    prio = fps_priority(N)
    temp = np.full((B, N), F32(1e10), F32)
    idx = np.zeros((B, npoint), np.int32)
    rows = np.arange(B)
    old = np.zeros(B, np.int64)
    r0 = 0
    if w is None:
        r0 = 1
    for r in range(r0, npoint):
        if w is not None and r == 0:
            old = _pick(w, prio)
        else:
            d = matrix[rows, old, :].astype(F32) if matrix is not None else sq_dist(src, src[rows, old][:, None, :])
            temp = np.minimum(d, temp)
            old = _pick(temp if w is None else weighted_rank(temp, w), prio)
        idx[:, r] = old
    return idx


def ball_query(xyz, new_xyz, nsample, r_out, r_in=0.0, chunk=512):
    """-> idx_cnt (B, M), idx (B, M, nsample) int32: the first nsample k with r_in^2 <= d2 < r_out^2, then repeated
    cyclically; an empty ball is all 0."""
    xyz, new_xyz = np.asarray(xyz, F32), np.asarray(new_xyz, F32)
    B, N = xyz.shape[:2]
    M = new_xyz.shape[1]
    ri2, ro2 = F32(r_in) * F32(r_in), F32(r_out) * F32(r_out)
    cnt = np.zeros((B, M), np.int32)
    idx = np.zeros((B, M, nsample), np.int32)
    slots = np.arange(nsample)
    for b in range(B):
        for q0 in range(0, M, chunk):
            d2 = sq_dist(new_xyz[b, q0:q0 + chunk, None, :], xyz[b, None, :, :])
            hit = (d2 >= ri2) & (d2 < ro2)
            first = np.argsort(~hit, axis=1, kind="stable")[:, :nsample]
            c = np.minimum(hit.sum(axis=1), nsample)
            cc = np.maximum(c, 1)
            sel = np.take_along_axis(first, slots[None, :] % cc[:, None], axis=1)
            idx[b, q0:q0 + chunk] = np.where(c[:, None] > 0, sel, 0)
            cnt[b, q0:q0 + chunk] = c
    return cnt, idx


def group_points(features, idx):
    """features (B, C, N), idx (B, M[, S]) -> (B, C, M[, S])."""
    features = np.asarray(features, F32)
    return np.stack([features[b][:, idx[b]] for b in range(features.shape[0])])


def three_nn(unknown, known):
    """-> dist2 (B, n, 3), idx (B, n, 3): strict-< insertion in ascending k (first index wins ties); unfilled slots
    (m < 3) hold inf and 0."""
    unknown, known = np.asarray(unknown, F32), np.asarray(known, F32)
    B, n = unknown.shape[:2]
    m = known.shape[1]
    dist2 = np.full((B, n, 3), np.inf, F32)
    idx = np.zeros((B, n, 3), np.int32)
    for b in range(B):
        for q0 in range(0, n, 1024):
            d = sq_dist(unknown[b, q0:q0 + 1024, None, :], known[b, None, :, :])
            order = np.argsort(d, axis=1, kind="stable")[:, :3]
            k = order.shape[1]
            dist2[b, q0:q0 + 1024, :k] = np.take_along_axis(d, order, axis=1)
            idx[b, q0:q0 + 1024, :k] = order
    return dist2, idx


def three_interpolate(features, idx, weight):
    """features (B, C, m), idx / weight (B, n, 3) -> (B, C, n) = ((w0*f0) + (w1*f1)) + (w2*f2)."""
    features, weight = np.asarray(features, F32), np.asarray(weight, F32)
    out = []
    for b in range(features.shape[0]):
        f = features[b][:, idx[b]]                     # (C, n, 3)
        p = (weight[b][None] * f).astype(F32)
        out.append((p[..., 0] + p[..., 1]) + p[..., 2])
    return np.stack(out)


# ------------------------------------------------------------------------------------------- direct simulations

def fps_simulate_reference(xyz, npoint, weights=None):
    """One frame, plain Python: the reference's thread scan (thread t scans k = t, t+bs, ..., keeping its first
    maximum over a start of -1) and its left-preferring LDS tree, round by round."""
    xyz = np.asarray(xyz, F32)
    n = xyz.shape[0]
    bs = 1 << fps_log2_bs(n)
    temp = [F32(1e10)] * n
    out, old = [], 0
    for j in range(npoint):
        if weights is None and j == 0:
            out.append(0)
            continue
        best, besti = [F32(-1)] * bs, [0] * bs
        for t in range(bs):
            for k in range(t, n, bs):
                if weights is not None and j == 0:
                    v = F32(weights[k])
                else:
                    temp[k] = min(F32(sq_dist(xyz[k], xyz[old])), temp[k])
                    v = temp[k] if weights is None else weighted_rank(np.array([temp[k]], F32),
                                                                      np.array([weights[k]], F32))[0]
                if v > best[t]:
                    best[t], besti[t] = v, k
        s = bs // 2
        while s >= 1:
            for t in range(s):
                if best[t + s] > best[t]:
                    best[t], besti[t] = best[t + s], besti[t + s]
            s //= 2
        old = besti[0]
        out.append(old)
    return np.array(out, np.int32)


def ball_query_scan(xyz, new_xyz, nsample, r_out, r_in=0.0):
    """One frame, plain Python: the per-query scan with early stop and cyclic padding."""
    ri2, ro2 = F32(r_in) * F32(r_in), F32(r_out) * F32(r_out)
    cnts, rows = [], []
    for q in np.asarray(new_xyz, F32):
        row = [0] * nsample
        cnt = 0
        for k, p in enumerate(np.asarray(xyz, F32)):
            d2 = sq_dist(q, p)
            if ri2 <= d2 < ro2:
                row[cnt] = k
                cnt += 1
                if cnt >= nsample:
                    break
        cnts.append(cnt)
        c, l = cnt, 0
        while c < nsample:
            row[c] = row[l]
            c += 1
            l += 1
        rows.append(row)
    return np.array(cnts, np.int32), np.array(rows, np.int32)
