"""Float32 numpy restatement of the stacked point ops (include/spx.h §18, csrc/pointnet2_stack.hip), written from their
stated semantics.  A helper module for the tests, not a test file.

Tensors are stacked over the frames, (N1 + N2 + ..., C), with one count per frame; rows past the sum of the counts are
dead.  Every float32 operation rounds once, exactly like the uncontracted kernels (pointnet2_ref.sq_dist).  The second
half holds plain-Python per-thread simulations of the reference's own scans."""
import numpy as np

from pointnet2_ref import F32, _bitrev, _pick, sq_dist

FPS_THREADS = 1024   # the reference launches the stack FPS with 1024 threads whatever the frame's size


def frame_starts(cnt, rows):
    """counts (B,) -> starts (B + 1,): exclusive prefix sums of max(cnt, 0), clamped to `rows`; starts[B] = live rows."""
    acc = np.concatenate([[0], np.cumsum(np.maximum(np.asarray(cnt, np.int64), 0))])
    return np.minimum(acc, rows).astype(np.int64)


def ball_query(xyz, xyz_cnt, new_xyz, new_cnt, radius, nsample, chunk=512):
    """-> idx (M, nsample) int32 frame-local, empty (M,) bool: the first nsample k (ascending) of the query's frame with
    d2 < radius*radius, unfilled slots = the first hit, an empty ball all 0 and empty = True; dead rows the same."""
    xyz, new_xyz = np.asarray(xyz, F32).reshape(-1, 3), np.asarray(new_xyz, F32).reshape(-1, 3)
    sn, sm = frame_starts(xyz_cnt, xyz.shape[0]), frame_starts(new_cnt, new_xyz.shape[0])
    r2 = F32(radius) * F32(radius)
    idx = np.zeros((new_xyz.shape[0], nsample), np.int32)
    empty = np.ones((new_xyz.shape[0],), bool)
    for f in range(len(sn) - 1):
        pts = xyz[sn[f]:sn[f + 1]]
        if pts.shape[0] == 0:
            continue
        for q0 in range(sm[f], sm[f + 1], chunk):
            q1 = min(q0 + chunk, sm[f + 1])
            hit = sq_dist(new_xyz[q0:q1, None, :], pts[None, :, :]) < r2
            first = np.argsort(~hit, axis=1, kind="stable")[:, :nsample]
            if first.shape[1] < nsample:
                first = np.concatenate([first, np.zeros((q1 - q0, nsample - first.shape[1]), first.dtype)], axis=1)
            c = np.minimum(hit.sum(axis=1), nsample)
            sel = np.where(np.arange(nsample)[None, :] < c[:, None], first, first[:, :1])
            idx[q0:q1] = np.where(c[:, None] > 0, sel, 0)
            empty[q0:q1] = c == 0
    return idx, empty


def _frame_of_rows(starts, rows):
    """frame of every row (rows,), -1 for dead rows"""
    r = np.arange(rows)
    f = np.searchsorted(starts[1:], r, side="right")
    return np.where(r < starts[-1], f, -1)


def global_rows(idx, feat_cnt, n_rows, idx_cnt):
    """frame-local idx (M, S) -> global source rows (M, S), -1 where the index is outside its frame or the row is dead"""
    idx = np.asarray(idx, np.int64)
    sn, sm = frame_starts(feat_cnt, n_rows), frame_starts(idx_cnt, idx.shape[0])
    f = _frame_of_rows(sm, idx.shape[0])
    fs = np.maximum(f, 0)
    start, size = sn[fs][:, None], (sn[fs + 1] - sn[fs])[:, None]
    ok = (f >= 0)[:, None] & (idx >= 0) & (idx < size)
    return np.where(ok, start + idx, -1)


def group_points(features, feat_cnt, idx, idx_cnt):
    """features (N, C), idx (M, S) frame-local -> (M, C, S); bad indices and dead rows give 0."""
    features = np.asarray(features, F32)
    rows = global_rows(idx, feat_cnt, features.shape[0], idx_cnt)
    if features.shape[0] == 0:
        return np.zeros((rows.shape[0], features.shape[1], rows.shape[1]), F32)
    out = features[np.maximum(rows, 0)]                                  # (M, S, C)
    out = np.where((rows >= 0)[:, :, None], out, F32(0))
    return np.ascontiguousarray(out.transpose(0, 2, 1)).astype(F32)


def three_nn(unknown, unknown_cnt, known, known_cnt):
    """-> dist2 (N, 3), idx (N, 3) GLOBAL known rows: strict-< insertion in ascending k (the first index wins ties);
    unfilled slots hold inf and the frame start; dead rows hold inf and 0."""
    unknown, known = np.asarray(unknown, F32).reshape(-1, 3), np.asarray(known, F32).reshape(-1, 3)
    sn, sm = frame_starts(unknown_cnt, unknown.shape[0]), frame_starts(known_cnt, known.shape[0])
    dist2 = np.full((unknown.shape[0], 3), np.inf, F32)
    idx = np.zeros((unknown.shape[0], 3), np.int32)
    for f in range(len(sn) - 1):
        idx[sn[f]:sn[f + 1]] = sm[f]
        kn = known[sm[f]:sm[f + 1]]
        if kn.shape[0] == 0:
            continue
        for q0 in range(sn[f], sn[f + 1], 1024):
            q1 = min(q0 + 1024, sn[f + 1])
            d = sq_dist(unknown[q0:q1, None, :], kn[None, :, :])
            order = np.argsort(d, axis=1, kind="stable")[:, :3]
            k = order.shape[1]
            dist2[q0:q1, :k] = np.take_along_axis(d, order, axis=1)
            idx[q0:q1, :k] = sm[f] + order
    return dist2, idx


def three_interpolate(features, idx, weight, cnt=None):
    """features (M, C), idx (global) / weight (N, 3) -> (N, C) = ((w0*f0) + (w1*f1)) + (w2*f2); an index outside
    [0, M) reads as 0; with cnt, the rows past its sum are 0."""
    features, weight, idx = np.asarray(features, F32), np.asarray(weight, F32), np.asarray(idx, np.int64)
    ok = (idx >= 0) & (idx < features.shape[0])
    if features.shape[0]:
        f = np.where(ok[:, :, None], features[np.where(ok, idx, 0)], F32(0))   # (N, 3, C)
    else:
        f = np.zeros(idx.shape + (features.shape[1],), F32)
    with np.errstate(invalid="ignore"):
        p = (weight[:, :, None] * f).astype(F32)
        out = ((p[:, 0] + p[:, 1]) + p[:, 2]).astype(F32)
    if cnt is not None:
        out[frame_starts(cnt, idx.shape[0])[-1]:] = 0
    return out


def fps_priority(n):
    """Tie priority of every point of a frame (smaller wins): (bitrev10(k mod 1024), k div 1024)."""
    k = np.arange(n, dtype=np.int64)
    return (_bitrev(k & (FPS_THREADS - 1), 10) << 32) | (k >> 10)


def stack_furthest_point_sample(xyz, xyz_cnt, npoint):
    """xyz (N, 3), counts (B,), npoint (B,) -> (sum npoint,) int32 GLOBAL rows.  The first pick of a frame is its first
    row; a frame without points picks its frame start every time."""
    xyz = np.asarray(xyz, F32).reshape(-1, 3)
    sn = frame_starts(xyz_cnt, xyz.shape[0])
    out = []
    for f, m in enumerate(npoint):
        pts = xyz[sn[f]:sn[f + 1]]
        n = pts.shape[0]
        picks = np.zeros((m,), np.int64)
        if n > 0:
            prio = fps_priority(n)
            temp = np.full((1, n), F32(1e10), F32)
            old = 0
            for r in range(1, m):
                temp = np.minimum(sq_dist(pts, pts[old])[None, :], temp)
                old = int(_pick(temp, prio)[0])
                picks[r] = old
        out.append(sn[f] + picks)
    return np.concatenate(out).astype(np.int32) if out else np.zeros((0,), np.int32)


# ------------------------------------------------------------------------------------------- direct simulations

def ball_query_simulate_reference(xyz, xyz_cnt, new_xyz, new_cnt, radius, nsample):
    """Plain Python, one reference thread per query (ball_query_kernel_stack): the frame search over the counts, the
    scan that fills EVERY slot with the first hit and then overwrites slot after slot, the -1 mark of an empty ball; then
    BallQuery.forward's fix-up (mask = idx[:, 0] == -1, idx[mask] = 0).  The tensors are exactly sized (no dead rows)."""
    xyz, new_xyz = np.asarray(xyz, F32).reshape(-1, 3), np.asarray(new_xyz, F32).reshape(-1, 3)
    B, M = len(new_cnt), new_xyz.shape[0]
    radius2 = F32(radius) * F32(radius)
    idx = np.zeros((M, nsample), np.int32)
    for pt_idx in range(M):
        bs_idx, pt_cnt = 0, int(new_cnt[0])
        for k in range(1, B):
            if pt_idx < pt_cnt:
                break
            pt_cnt += int(new_cnt[k])
            bs_idx = k
        start = int(sum(int(c) for c in xyz_cnt[:bs_idx]))
        n = int(xyz_cnt[bs_idx])
        q = new_xyz[pt_idx]
        cnt = 0
        for k in range(n):
            d2 = sq_dist(q, xyz[start + k])
            if d2 < radius2:
                if cnt == 0:
                    for l in range(nsample):
                        idx[pt_idx, l] = k
                idx[pt_idx, cnt] = k
                cnt += 1
                if cnt >= nsample:
                    break
        if cnt == 0:
            idx[pt_idx, 0] = -1
    empty = idx[:, 0] == -1
    idx[empty] = 0
    return idx, empty


def fps_simulate_reference(xyz, xyz_cnt, npoint):
    """Plain Python, stack_farthest_point_sampling_kernel<1024>: per frame, thread t scans k = t, t + 1024, ..., keeping
    its first maximum over a start of (-1, 0), then the left-preferring LDS tree, round by round.  Frames must hold at
    least one point (the reference reads out of bounds otherwise)."""
    xyz = np.asarray(xyz, F32).reshape(-1, 3)
    out, start = [], 0
    for f, m in enumerate(npoint):
        n = int(xyz_cnt[f])
        pts = xyz[start:start + n]
        temp = np.full((n,), F32(1e10), F32)
        old = 0
        if m > 0:
            out.append(start)
        for _ in range(1, m):
            temp = np.minimum(sq_dist(pts, pts[old]), temp)
            tl = temp.tolist()
            best, besti = [-1.0] * FPS_THREADS, [0] * FPS_THREADS
            for t in range(min(FPS_THREADS, n)):
                for k in range(t, n, FPS_THREADS):
                    if tl[k] > best[t]:
                        best[t], besti[t] = tl[k], k
            s = FPS_THREADS // 2
            while s >= 1:
                for t in range(s):
                    if best[t + s] > best[t]:
                        best[t], besti[t] = best[t + s], besti[t + s]
                s //= 2
            old = besti[0]
            out.append(start + old)
        start += n
    return np.array(out, np.int32)
