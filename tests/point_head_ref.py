"""Float64 restatement of the fast_cpc point head's eval vote step and tail (csrc/point_head.hip, include/spx.h §14),
and a literal transcription of the reference's eval forward on a head module's own submodules (reference
point_head_vote_sasa_statistic_distillation.py, forward with self.training False, student branch).

MLP parameters are (w1 (H, C), bn_mean, bn_var, bn_weight, bn_bias (H), eps, w2 (O, H), b2 (O)).  The restatement also
returns, per output, the absolute sum sum|w . x| through both layers, the scale that fp32 rounding error follows."""
import numpy as np
import torch


def mlp_params(seq, dtype=np.float64):
    """Sequential(Conv1d, BatchNorm1d, ReLU, Conv1d) -> numpy parameter tuple."""
    c1, bn, _, c2 = seq

    def a(t):
        return t.detach().cpu().numpy().astype(dtype)

    return (a(c1.weight).reshape(c1.weight.shape[0], -1), a(bn.running_mean), a(bn.running_var), a(bn.weight),
            a(bn.bias), float(bn.eps), a(c2.weight).reshape(c2.weight.shape[0], -1), a(c2.bias))


def _mlp(x, p, stat=None):
    """x (C, M) -> y (O, M), |y| scale (O, M)."""
    w1, mean, var, gamma, beta, eps, w2, b2 = p
    if stat is not None:
        x = x * stat[:, None]
    pre = w1 @ x
    pre_abs = np.abs(w1) @ np.abs(x)
    scale = gamma / np.sqrt(var + eps)
    h = np.maximum((pre - mean[:, None]) * scale[:, None] + beta[:, None], 0.0)
    h_abs = (pre_abs + np.abs(mean)[:, None]) * np.abs(scale)[:, None] + np.abs(beta)[:, None]
    return w2 @ h + b2[:, None], np.abs(w2) @ h_abs + np.abs(b2)[:, None]


def vote(feat, xyz, lo, hi, p, max_range):
    """feat (B, C, N), xyz (B, N, 3) -> vote (B, nv, 3), |.| scale of the offset (B, nv, 3)."""
    feat, xyz = np.asarray(feat, np.float64), np.asarray(xyz, np.float64)
    b, c, n = feat.shape
    lo, hi, _ = slice(lo, hi).indices(n)
    x = feat[:, :, lo:hi].transpose(1, 0, 2).reshape(c, -1)
    off, off_abs = _mlp(x, p)
    r = np.asarray(max_range, np.float64)[:, None]
    off = np.minimum(np.maximum(off, -r), r)
    nv = hi - lo
    off = off.reshape(3, b, nv).transpose(1, 2, 0)
    return xyz[:, lo:hi] + off, off_abs.reshape(3, b, nv).transpose(1, 2, 0)


def decode(reg, xyz, bins):
    """PointBinResidualCoder.decode_torch with use_mean_size False, in float64; the bin is the first maximum."""
    cls = reg[:, 6:6 + bins]
    k = np.argmax(cls, axis=1)
    res = reg[:, 6 + bins:6 + 2 * bins][np.arange(reg.shape[0]), k]
    ang = (k + res) * (2 * np.pi / bins)
    return np.concatenate([reg[:, 0:3] + xyz, np.exp(reg[:, 3:6]), ang[:, None]], axis=1), k


def predict(feat, stat, vote_xyz, cls_params, reg_params, bins):
    """feat (B, C, N), stat (K, C), vote_xyz (B * N, 3) -> dict of cls (B * N, K), reg (B * N, 6 + 2 bins),
    box (B * N, 7), bin (B * N), cls_abs, reg_abs (the |.| scales)."""
    feat = np.asarray(feat, np.float64)
    stat = np.asarray(stat, np.float64)
    b, c, n = feat.shape
    x = feat.transpose(1, 0, 2).reshape(c, -1)          # column m = bi * n + i
    cls, cls_abs = [], []
    for k, p in enumerate(cls_params):
        y, ya = _mlp(x, p, stat[k])
        cls.append(y[0])
        cls_abs.append(ya[0])
    reg, reg_abs = _mlp(x, reg_params)
    reg, reg_abs = reg.T, reg_abs.T
    box, kbin = decode(reg, np.asarray(vote_xyz, np.float64), bins)
    return dict(cls=np.stack(cls, 1), cls_abs=np.stack(cls_abs, 1), reg=reg, reg_abs=reg_abs, box=box, bin=kbin)


# ------------------------------------------------------------------- literal transcription of the reference (torch)
def transcribe_vote(head, s_point_coords, s_point_features, batch_size):
    """Reference forward up to s_vote_coords (eval, student), on the head's own s_vote_layers.  Returns the
    candidate coords (B, nv, 3), vote coords (B, nv, 3) and sample batch index (B, nv, 1)."""
    s_batch_idx, coords = s_point_coords[:, 0], s_point_coords[:, 1:4]
    s_batch_idx = s_batch_idx.view(batch_size, -1, 1)
    coords = coords.view(batch_size, -1, 3).contiguous()
    feats = s_point_features.reshape(batch_size, coords.size(1), -1).permute(0, 2, 1).contiguous()
    sample_range = head.model_cfg.SAMPLE_RANGE
    s_sample_batch_idx = s_batch_idx[:, sample_range[0]:sample_range[1], :].contiguous()
    cand = coords[:, sample_range[0]:sample_range[1], :].contiguous()
    cand_f = feats[:, :, sample_range[0]:sample_range[1]].contiguous()
    off = head.s_vote_layers(cand_f)
    rng = torch.tensor(np.array(head.s_vote_cfg.MAX_TRANSLATION_RANGE, dtype=np.float32), dtype=off.dtype,
                       device=off.device).unsqueeze(0).unsqueeze(-1)
    off = torch.max(off, -rng)
    off = torch.min(off, rng)
    return cand, cand + off.permute(0, 2, 1).contiguous(), s_sample_batch_idx


def transcribe_tail(head, s_point_features, s_vote_coords_flat):
    """Reference forward after s_shared_fc_layer (eval, student): the statistic-modulated class blocks, s_reg_layers,
    the decode of s_point_box_preds and generate_predicted_boxes.  Returns (cls_preds, reg_preds, box_preds,
    batch_box_preds)."""
    batch_size, _, npp = s_point_features.shape
    num = batch_size * npp
    res = []
    for i in range(head.num_class):
        stat = head.object_statistic_features[i:(i + 1), :]
        r = head.s_cls_block[i](s_point_features * stat.unsqueeze(-1))
        res.append(r.permute(0, 2, 1).contiguous().view(num, -1))
    cls_preds = torch.cat(res, dim=-1)
    reg = head.s_reg_layers(s_point_features)
    reg = reg.permute(0, 2, 1).contiguous()
    reg = reg.view(-1, reg.shape[-1]).contiguous()
    box = head.box_coder.decode_torch(reg, s_vote_coords_flat)
    _, pred_classes = cls_preds.max(dim=-1)
    batch_box = head.box_coder.decode_torch(reg, s_vote_coords_flat, pred_classes + 1)
    return cls_preds, reg, box, batch_box
