"""ResidualCoder — SECOND's anchor-relative box code (semantics of reference pcdet/utils/box_coder_utils.py:5-79);
PointBinResidualCoder — the point-relative, angle-bin code of the 3DSSD point heads (reference :225-363)."""
import numpy as np
import torch


class ResidualCoder(object):
    def __init__(self, code_size=7, encode_angle_by_sincos=False, **kwargs):
        self.code_size = code_size + (1 if encode_angle_by_sincos else 0)
        self.encode_angle_by_sincos = encode_angle_by_sincos

    def encode_torch(self, boxes, anchors):
        """boxes, anchors (..., 7+C) [x,y,z,dx,dy,dz,heading,...] -> residual code (..., code_size).
        Sizes are clamped to >= 1e-5 (on copies: the reference clamps its arguments in place)."""
        a_xyz, a_sz, a_r, a_rest = anchors[..., 0:3], anchors[..., 3:6].clamp_min(1e-5), anchors[..., 6:7], anchors[..., 7:]
        g_xyz, g_sz, g_r, g_rest = boxes[..., 0:3], boxes[..., 3:6].clamp_min(1e-5), boxes[..., 6:7], boxes[..., 7:]
        diag = torch.sqrt(a_sz[..., 0:1] ** 2 + a_sz[..., 1:2] ** 2)
        t_xy = (g_xyz[..., 0:2] - a_xyz[..., 0:2]) / diag
        t_z = (g_xyz[..., 2:3] - a_xyz[..., 2:3]) / a_sz[..., 2:3]
        t_sz = torch.log(g_sz / a_sz)
        if self.encode_angle_by_sincos:
            t_r = torch.cat([torch.cos(g_r) - torch.cos(a_r), torch.sin(g_r) - torch.sin(a_r)], dim=-1)
        else:
            t_r = g_r - a_r
        return torch.cat([t_xy, t_z, t_sz, t_r, g_rest - a_rest], dim=-1)

    def decode_torch(self, box_encodings, anchors):
        """inverse of encode_torch; (B,N,7+C) or (N,7+C)."""
        a_xyz, a_sz, a_r, a_rest = anchors[..., 0:3], anchors[..., 3:6], anchors[..., 6:7], anchors[..., 7:]
        t = box_encodings
        diag = torch.sqrt(a_sz[..., 0:1] ** 2 + a_sz[..., 1:2] ** 2)
        g_xy = t[..., 0:2] * diag + a_xyz[..., 0:2]
        g_z = t[..., 2:3] * a_sz[..., 2:3] + a_xyz[..., 2:3]
        g_sz = torch.exp(t[..., 3:6]) * a_sz
        if self.encode_angle_by_sincos:
            g_r = torch.atan2(t[..., 7:8] + torch.sin(a_r), t[..., 6:7] + torch.cos(a_r))
            rest = t[..., 8:]
        else:
            g_r = t[..., 6:7] + a_r
            rest = t[..., 7:]
        return torch.cat([g_xy, g_z, g_sz, g_r, rest + a_rest], dim=-1)


class PointBinResidualCoder(object):
    """Point-relative box code with a classified heading: [x, y, z, log dx, log dy, log dz, bin one-hot (B),
    bin residual (B), extra...].  Unlike the reference, mean_size stays on the host at construction and is moved to
    the device of the inputs when used, so the coder builds on a CPU-only machine."""

    def __init__(self, code_size=30, use_mean_size=True, angle_bin_num=12, pred_velo=False, **kwargs):
        super().__init__()
        self.code_size = 6 + 2 * angle_bin_num
        self.angle_bin_num = angle_bin_num
        self.pred_velo = pred_velo
        if pred_velo:
            self.code_size += 2
        self.use_mean_size = use_mean_size
        if self.use_mean_size:
            self.mean_size = torch.from_numpy(np.array(kwargs['mean_size'])).float()
            assert self.mean_size.min() > 0

    def _mean_size(self, device):
        return self.mean_size.to(device)

    def encode_angle_torch(self, angle):
        """angle (N) -> angle_cls (N, B) one-hot, angle_res (N, B) normalised residual in its bin's slot."""
        angle = torch.remainder(angle, np.pi * 2.0)
        angle_per_class = np.pi * 2.0 / float(self.angle_bin_num)
        shifted_angle = torch.remainder(angle + angle_per_class / 2.0, np.pi * 2.0)

        angle_cls_f = (shifted_angle / angle_per_class).floor()
        angle_cls = angle_cls_f.new_zeros(*list(angle_cls_f.shape), self.angle_bin_num)
        angle_cls.scatter_(-1, angle_cls_f.unsqueeze(-1).long(), 1.0)

        angle_res = shifted_angle - (angle_cls_f * angle_per_class + angle_per_class / 2.0)
        angle_res = angle_res / angle_per_class
        angle_res = angle_cls * angle_res.unsqueeze(-1)
        return angle_cls, angle_res

    def decode_angle_torch(self, angle_cls, angle_res):
        """angle_cls, angle_res (N, B) -> angle (N); the bin is the first maximum of angle_cls."""
        angle_cls_idx = angle_cls.argmax(dim=-1)
        angle_cls_onehot = angle_cls.new_zeros(angle_cls.shape)
        angle_cls_onehot.scatter_(-1, angle_cls_idx.unsqueeze(-1), 1.0)

        angle_res = (angle_cls_onehot * angle_res).sum(dim=-1)
        angle = (angle_cls_idx.float() + angle_res) * (np.pi * 2.0 / float(self.angle_bin_num))
        return angle

    def encode_torch(self, gt_boxes, points, gt_classes=None):
        """gt_boxes (N, 7 + C) [x, y, z, dx, dy, dz, heading, ...] (sizes clamped to >= 1e-5 IN PLACE, as the
        reference does), points (N, 3), gt_classes (N) in [1, num_classes] -> box_coding (N, 6 + 2 * B + C)."""
        gt_boxes[:, 3:6] = torch.clamp_min(gt_boxes[:, 3:6], min=1e-5)

        xg, yg, zg, dxg, dyg, dzg, rg, *cgs = torch.split(gt_boxes, 1, dim=-1)
        xa, ya, za = torch.split(points, 1, dim=-1)

        if self.use_mean_size:
            mean_size = self._mean_size(gt_boxes.device)
            assert gt_classes.max() <= mean_size.shape[0]
            point_anchor_size = mean_size[gt_classes - 1]
            dxa, dya, dza = torch.split(point_anchor_size, 1, dim=-1)
            diagonal = torch.sqrt(dxa ** 2 + dya ** 2)
            xt = (xg - xa) / diagonal
            yt = (yg - ya) / diagonal
            zt = (zg - za) / dza
            dxt = torch.log(dxg / dxa)
            dyt = torch.log(dyg / dya)
            dzt = torch.log(dzg / dza)
        else:
            xt = (xg - xa)
            yt = (yg - ya)
            zt = (zg - za)
            dxt = torch.log(dxg)
            dyt = torch.log(dyg)
            dzt = torch.log(dzg)

        rg_cls, rg_reg = self.encode_angle_torch(rg.squeeze(-1))
        cts = [g for g in cgs]
        return torch.cat([xt, yt, zt, dxt, dyt, dzt, rg_cls, rg_reg, *cts], dim=-1)

    def decode_torch_kernel(self, box_offsets, box_angle_cls, box_angle_reg, points, pred_classes=None):
        """box_offsets (N, 6), box_angle_cls / box_angle_reg (N, B), points (N, 3), pred_classes (N) in
        [1, num_classes] (use_mean_size only) -> boxes3d (N, 7)."""
        xt, yt, zt, dxt, dyt, dzt = torch.split(box_offsets, 1, dim=-1)
        xa, ya, za = torch.split(points, 1, dim=-1)

        if self.use_mean_size:
            mean_size = self._mean_size(box_offsets.device)
            assert pred_classes.max() <= mean_size.shape[0]
            point_anchor_size = mean_size[pred_classes - 1]
            dxa, dya, dza = torch.split(point_anchor_size, 1, dim=-1)
            diagonal = torch.sqrt(dxa ** 2 + dya ** 2)
            xg = xt * diagonal + xa
            yg = yt * diagonal + ya
            zg = zt * dza + za

            dxg = torch.exp(dxt) * dxa
            dyg = torch.exp(dyt) * dya
            dzg = torch.exp(dzt) * dza
        else:
            xg = xt + xa
            yg = yt + ya
            zg = zt + za
            dxg = torch.exp(dxt)
            dyg = torch.exp(dyt)
            dzg = torch.exp(dzt)

        rg = self.decode_angle_torch(box_angle_cls, box_angle_reg).unsqueeze(-1)
        return torch.cat([xg, yg, zg, dxg, dyg, dzg, rg], dim=-1)

    def decode_torch(self, box_encodings, points, pred_classes=None):
        """box_encodings (N, 6 + 2 * B + C), points (N, 3), pred_classes (N) -> boxes3d (N, 7 + C)."""
        box_offsets = box_encodings[:, :6]
        box_angle_cls = box_encodings[:, 6:6 + self.angle_bin_num]
        box_angle_reg = box_encodings[:, 6 + self.angle_bin_num:6 + self.angle_bin_num * 2]
        cgs = box_encodings[:, 6 + self.angle_bin_num * 2:]

        boxes3d = self.decode_torch_kernel(box_offsets, box_angle_cls, box_angle_reg, points, pred_classes)
        return torch.cat([boxes3d, cgs], dim=-1)
