"""hipGraph-captured, host-sync-free inference forward (MI355X-first execution model).

The reference's forward (pcdet/models/detectors/second_net.py:9-22) launches ~150 kernels per batch and — through spconv
— synchronises with the host for every data-dependent size (number of voxels, active outputs of each strided conv).
Here every libspx kernel can read its live row count from device memory (include/spx.h, the `d_n*` arguments), so the
whole path  points -> voxelise -> 12 sparse convs (+ fused BN/ReLU) -> densify -> BEV backbone -> anchor head decode
runs at static CAPACITY shapes without a single host sync and is captured once into a hipGraph
(torch.cuda.CUDAGraph); each call is a copy into the static point buffer plus one graph replay.

Capacities: voxels = min(max_points, batch * MAX_NUMBER_OF_VOXELS['test']); the output rows of each strided conv default
to `level_factors` x the voxel capacity (LiDAR scenes shrink after the first stride-2 stage; the no-overflow bound is 8x
per stage).  Rows beyond a capacity are dropped and reported by `overflowed()` (reads the device counters: one sync, call
it when convenient).
"""
import os

import torch

from spx.functional import refresh_folded_bn, refresh_graph_constants

DEFAULT_LEVEL_FACTORS = {'spconv2': 2.0, 'spconv3': 2.0, 'spconv4': 1.0, 'spconv_down2': 1.0}


def static_caps_for(model, batch_size, n_points, training=None, level_factors=None):
    """Row capacities for the host-sync-free (static-capacity) execution of `model` on batches of at most `n_points`
    points: put the returned dict in batch_dict['static_caps'] (training or eval).  The voxel capacity is exact — the
    reference's hard cap min(points, batch * MAX_NUMBER_OF_VOXELS[mode]); the output rows of each strided conv get
    `level_factors` x that (the no-overflow bound is 8x per stage and would size every later kernel for rows that never
    exist).  An overflow never passes silently: the rule-table kernels raise SPX_ERR_CAPACITY in the device status word
    (spx.ops.check_status) and the live counts stay readable in the tensors' n_valid."""
    training = model.training if training is None else training
    vox_cap = min(int(n_points), int(batch_size) * int(model.vfe.max_voxels['train' if training else 'test']))
    f = dict(DEFAULT_LEVEL_FACTORS)
    f.update(level_factors or {})
    caps = {k: max(1, int(v * vox_cap)) for k, v in f.items()}
    caps['voxels'] = vox_cap
    return caps


class GraphedDetector(object):
    def __init__(self, model, batch_size, max_points, level_factors=None, warmup=2, n_modules=None):
        """n_modules: run only the first n modules of model.module_list (3 = voxelise + VFE, 3-D backbone, BEV collapse)."""
        self.model = model.eval()
        self.modules = list(model.module_list) if n_modules is None else list(model.module_list)[:int(n_modules)]
        self.batch_size = int(batch_size)
        vfe = model.vfe
        self.device = next(model.parameters()).device
        assert self.device.type == 'cuda'
        c = 1 + vfe.num_point_features
        self.max_points = int(max_points)
        self.points = torch.empty((self.max_points, c), dtype=torch.float32, device=self.device)
        self._pad_row = torch.zeros((c,), dtype=torch.float32, device=self.device)
        self._pad_row[0] = self.batch_size - 1                       # keeps frame ids ascending
        self._pad_row[1] = float(vfe.point_cloud_range[0]) - 1.0e4   # far outside the range: dropped by the voxeliser
        self.points[:] = self._pad_row
        vox_cap = min(self.max_points, self.batch_size * int(vfe.max_voxels['test']))
        f = dict(DEFAULT_LEVEL_FACTORS)
        f.update(level_factors or {})
        self.static_caps = {k: max(1, int(v * vox_cap)) for k, v in f.items()}
        self.vox_cap = vox_cap
        self.out = None
        # eager warm-up on a side stream (allocator pools, workspaces, MIOpen kernel selection), then capture
        s = torch.cuda.Stream(device=self.device)
        s.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(s):
            for _ in range(warmup):
                self._forward()
        torch.cuda.current_stream(self.device).wait_stream(s)
        torch.cuda.synchronize(self.device)
        self.graph = torch.cuda.CUDAGraph()
        dot = os.environ.get("SPX_GRAPH_DOT")           # dev knob: write the captured graph (nodes + dependencies) as DOT
        if dot:
            self.graph.enable_debug_mode()
        with torch.cuda.graph(self.graph):
            self.out = self._forward()
        if dot:
            self.graph.debug_dump(dot)

    def _forward(self):
        bd = {'points': self.points, 'batch_size': self.batch_size, 'static_caps': self.static_caps}
        with torch.no_grad():
            for m in self.modules:
                bd = m(bd)
        ms = bd['multi_scale_3d_features']
        out = {k: bd[k] for k in ('batch_cls_preds', 'batch_box_preds', 'cls_preds_normalized') if k in bd}
        out.update({'batch_size': self.batch_size,
                'spatial_features': bd['spatial_features'],
                'counts': {'voxels': bd['voxel_num_valid'], 'spconv2': ms['x_conv2'].n_valid,
                           'spconv3': ms['x_conv3'].n_valid, 'spconv4': ms['x_conv4'].n_valid,
                           'spconv_down2': bd['encoded_spconv_tensor'].n_valid}})
        return out

    def __call__(self, points):
        """points [N, 1+C] (frame index in column 0, frames contiguous and ascending), N <= max_points, on the GPU.
        Returns the static output dict (overwritten by the next call)."""
        n = points.shape[0]
        if n > self.max_points:
            raise ValueError("%d points > capacity %d" % (n, self.max_points))
        self.points[:n].copy_(points, non_blocking=True)
        if n < self.max_points:
            self.points[n:] = self._pad_row
        refresh_folded_bn(self.model)        # BatchNorm folds the graph captured: rebuilt in place if a parameter was written
        refresh_graph_constants()            # likewise the packed weights / Winograd images it reads
        self.graph.replay()
        return self.out

    def overflowed(self):
        """{level: (live count, capacity)} for every level whose capacity was exceeded in the LAST call (one host sync)."""
        caps = dict(self.static_caps, voxels=self.vox_cap)
        bad = {}
        for k, t in self.out['counts'].items():
            v = int(t.item())
            if v > caps[k]:
                bad[k] = (v, caps[k])
        return bad

    def post_process(self):
        """score threshold + NMS on the last outputs (data dependent: outside the graph)."""
        return self.model.post_processing(dict(self.out))


class GraphedCenterPoint(GraphedDetector):
    """Eval forward of CenterPoint WITH its box decoding, NMS and (optionally) recall counts as ONE hipGraph replay.

    Same static point buffer, padding row, row capacities, warm-up and capture as GraphedDetector; in static mode the
    centre head decodes through CenterHead.generate_predicted_boxes_static (spx.ops.center_decode +
    spx.ops.point_post_process, no host read) and CenterPoint.post_processing_static adds the recall counts, so the
    whole chain is captured.  That the capture succeeds is itself the check that no host read is left on the path.

    max_gt > 0 keeps a static (batch_size, max_gt, gt_columns) ground-truth buffer, zero padded, and the graph then
    holds spx.ops.recall_count as well: pass gt_boxes to the call."""

    def __init__(self, model, batch_size, max_points, level_factors=None, warmup=2, max_gt=0, gt_columns=8):
        device = next(model.parameters()).device
        self.max_gt = int(max_gt)
        self.gt_boxes = None
        if self.max_gt > 0:
            self.gt_boxes = torch.zeros((int(batch_size), self.max_gt, int(gt_columns)), dtype=torch.float32, device=device)
        super().__init__(model, batch_size, max_points, level_factors=level_factors, warmup=warmup)

    def _forward(self):
        """The eager static path: what the graph holds.  Returns CenterPoint.post_processing_static's dict plus the
        live row counts GraphedDetector.overflowed reads."""
        bd = {'points': self.points, 'batch_size': self.batch_size, 'static_caps': self.static_caps}
        if self.gt_boxes is not None:
            bd['gt_boxes'] = self.gt_boxes
        with torch.no_grad():
            for m in self.modules:
                bd = m(bd)
            out = dict(self.model.post_processing_static(bd))
        ms = bd['multi_scale_3d_features']
        out['batch_size'] = self.batch_size
        out['counts'] = {'voxels': bd['voxel_num_valid'], 'spconv2': ms['x_conv2'].n_valid,
                         'spconv3': ms['x_conv3'].n_valid, 'spconv4': ms['x_conv4'].n_valid,
                         'spconv_down2': bd['encoded_spconv_tensor'].n_valid}
        return out

    def __call__(self, points, gt_boxes=None):
        """Copies the batch in and replays.  Returns the static output dict (overwritten by the next call)."""
        if (gt_boxes is not None) != (self.gt_boxes is not None):
            raise ValueError("gt_boxes go with a runner built with max_gt > 0, and only with one")
        if gt_boxes is not None:
            if gt_boxes.shape[0] != self.batch_size or gt_boxes.shape[1] > self.max_gt \
                    or gt_boxes.shape[2] != self.gt_boxes.shape[2]:
                raise ValueError("gt_boxes %s do not fit the captured buffer %s"
                                 % (tuple(gt_boxes.shape), tuple(self.gt_boxes.shape)))
            self.gt_boxes.zero_()
            self.gt_boxes[:, :gt_boxes.shape[1]].copy_(gt_boxes, non_blocking=True)
        return super().__call__(points)

    def pred_dicts(self):
        """The last call's result as model(batch) returns it in eval: (pred_dicts, recall_dict).  One host read."""
        return self.model.pred_dicts_from_static(self.out)

    def post_process(self):
        return self.pred_dicts()


class GraphedAnchorDetector(GraphedDetector):
    """Eval forward of an anchor-head detector (SECOND, PointPillars) WITH its score threshold, top-K and NMS as ONE
    hipGraph replay.

    Same static point buffer, padding row, row capacities, warm-up and capture as GraphedDetector; the forward ends in
    Detector3DTemplate.post_processing_static, which serves the dense (B, anchors, .) predictions through
    spx.ops.dense_post_process (no host read) whatever POST_PROCESSING.FUSED says.  That the capture succeeds is itself
    the check that no host read is left on the path.  Without gt_boxes there is no recall record."""

    def _forward(self):
        """The eager static path: what the graph holds.  Returns post_processing_static's dict, the head's dense
        predictions it read and the live row counts of every capacity the modules report."""
        bd = {'points': self.points, 'batch_size': self.batch_size, 'static_caps': self.static_caps}
        with torch.no_grad():
            for m in self.modules:
                bd = m(bd)
            plan = self.model._fused_post_plan(bd, dense=True)
            if plan is None:
                raise NotImplementedError('GraphedAnchorDetector needs dense (B, N, .) predictions that '
                                          'Detector3DTemplate._dense_post_plan admits')
            out = dict(self.model.post_processing_static(bd, plan))
        out.update({k: bd[k] for k in ('batch_cls_preds', 'batch_box_preds', 'cls_preds_normalized')})
        out['batch_size'] = self.batch_size
        out['counts'] = {'voxels': bd['voxel_num_valid']}
        ms = bd.get('multi_scale_3d_features', None)
        if ms is not None:
            out['counts'].update({'spconv2': ms['x_conv2'].n_valid, 'spconv3': ms['x_conv3'].n_valid,
                                  'spconv4': ms['x_conv4'].n_valid,
                                  'spconv_down2': bd['encoded_spconv_tensor'].n_valid})
        return out

    def pred_dicts(self):
        """The last call's result as model.post_processing returns it: (pred_dicts, recall_dict).  One host read (the
        frames' counts and the live row counts); raises if a row capacity overflowed, the results are then those of a
        truncated scene."""
        st = self.out
        b = self.batch_size
        keys = sorted(st['counts'])
        host = torch.cat([st['count'].to(torch.int64)] + [st['counts'][k].reshape(-1)[:1].to(torch.int64) for k in keys]).tolist()
        caps = dict(self.static_caps, voxels=self.vox_cap)
        bad = {k: (v, caps[k]) for k, v in zip(keys, host[b:]) if v > caps[k]}
        if bad:
            raise RuntimeError("GraphedAnchorDetector: row capacities exceeded (live rows, capacity): %s" % bad)
        preds = [{'pred_boxes': st['pred_boxes'][i, :host[i]], 'pred_scores': st['pred_scores'][i, :host[i]],
                  'pred_labels': st['pred_labels'][i, :host[i]]} for i in range(b)]
        return preds, {}

    def post_process(self):
        return self.pred_dicts()


class GraphedPointDetector(object):
    """Eval forward of a point detector (Point3DSSD: VoxelPointNet2FSMSGDistillation backbone, vote head) with its
    post-processing as ONE hipGraph replay.

    The backbone's static mode (batch_dict['static_caps'], pointnet2_backbone.py) keeps every voxel tensor at the row
    capacity B * NPOINT_LIST[0] with the live count on the device, the head follows it and
    Detector3DTemplate.post_processing_static needs no host read either, so the whole chain is captured once; a call is
    a copy into the static point buffer plus one replay.  That the capture succeeds is itself the check that no host
    read is left on the path.

    Every frame must hold exactly points_per_frame points (the reference's sample_points pads by resampling): points is
    (batch_size * points_per_frame, 1 + C) with the frame index in column 0, frames contiguous and ascending."""

    def __init__(self, model, batch_size, points_per_frame, warmup=2, example=None):
        """example: points to warm up and capture on (the buffer otherwise holds every point at the centre of the
        range)."""
        if model.training:
            raise ValueError("GraphedPointDetector captures the inference forward: call model.eval() first")
        self.model = model
        self.batch_size, self.points_per_frame = int(batch_size), int(points_per_frame)
        if self.batch_size < 1 or self.points_per_frame < 1:
            raise ValueError("batch_size and points_per_frame must be positive")
        self.num_features = 1 + int(model.dataset.point_feature_encoder.num_point_features)
        if example is not None:
            self._check(example)
        self.device = next(model.parameters()).device
        if self.device.type != 'cuda':
            raise ValueError("GraphedPointDetector needs the model on a GPU")
        rows = self.batch_size * self.points_per_frame
        self.points = torch.zeros((rows, self.num_features), dtype=torch.float32, device=self.device)
        self.points[:, 0] = torch.arange(self.batch_size, device=self.device).repeat_interleave(self.points_per_frame)
        rng = torch.as_tensor([float(v) for v in model.dataset.point_cloud_range], device=self.device)
        self.points[:, 1:4] = 0.5 * (rng[0:3] + rng[3:6])
        if example is not None:
            self.points.copy_(example, non_blocking=True)
        self.out = None
        # eager warm-up on a side stream (allocator pools, workspaces, MIOpen kernel selection, cached constants), then capture
        s = torch.cuda.Stream(device=self.device)
        s.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(s):
            for _ in range(max(int(warmup), 1)):
                self._forward()
        torch.cuda.current_stream(self.device).wait_stream(s)
        torch.cuda.synchronize(self.device)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.out = self._forward()

    def _check(self, points):
        want = (self.batch_size * self.points_per_frame, self.num_features)
        if points.dim() != 2 or tuple(points.shape) != want:
            raise ValueError("GraphedPointDetector was captured for %d frames of exactly %d points with %d columns: "
                             "points must be %s, got %s (pad short frames by resampling)"
                             % (self.batch_size, self.points_per_frame, self.num_features, want, tuple(points.shape)))

    def _forward(self):
        """The eager static path: what the graph holds.  Returns post_processing_static's dict plus voxel_num_valid
        (device int64[1], live voxels of the backbone), static_flags (the backbone's device booleans) and the head's
        flat predictions post_processing reads (batch_index, batch_cls_preds, batch_box_preds, cls_preds_normalized)."""
        bd = {'points': self.points, 'batch_size': self.batch_size, 'static_caps': {}}
        with torch.no_grad():
            for m in self.model.module_list:
                bd = m(bd)
            out = dict(self.model.post_processing_static(bd))
        out['voxel_num_valid'] = bd['voxel_num_valid']
        out['static_flags'] = bd['static_flags']
        out.update({k: bd[k] for k in ('batch_index', 'batch_cls_preds', 'batch_box_preds', 'cls_preds_normalized')})
        out['batch_size'] = self.batch_size
        return out

    def __call__(self, points):
        """Copies the batch in and replays.  Returns the static output dict (overwritten by the next call)."""
        self._check(points)
        self.points.copy_(points, non_blocking=True)
        refresh_folded_bn(self.model)        # BatchNorm folds the graph captured: rebuilt in place if a parameter was written
        refresh_graph_constants()            # likewise the packed weights it reads
        self.graph.replay()
        return self.out

    def pred_dicts(self):
        """The last call's detections as model.post_processing returns them: a list of {'pred_boxes', 'pred_scores',
        'pred_labels'} per frame.  One host read (counts and flags); a False flag raises, the results of such a batch
        are meaningless."""
        st = self.out
        names = ['post-processing layout_ok'] + ['backbone ' + k for k in sorted(st['static_flags'])]
        flags = [st['layout_ok']] + [st['static_flags'][k] for k in sorted(st['static_flags'])]
        host = torch.cat([st['count'].to(torch.int64)] + [f.to(torch.int64).view(1) for f in flags]).tolist()
        b = self.batch_size
        bad = [n for n, v in zip(names, host[b:]) if not v]
        if bad:
            raise RuntimeError("GraphedPointDetector: the batch broke the static path's contract (%s is False): frames "
                               "must be equal, contiguous and ascending, and every sampled point inside "
                               "POINT_CLOUD_RANGE" % ", ".join(bad))
        return [{'pred_boxes': st['pred_boxes'][i, :host[i]], 'pred_scores': st['pred_scores'][i, :host[i]],
                 'pred_labels': st['pred_labels'][i, :host[i]]} for i in range(b)]


class GraphedTrainStep(object):
    """Forward + backward of one training step as ONE hipGraph replay (single process; data-parallel ranks stay eager: DDP's
    bucket hooks and the RCCL all-reduce are not captured here).

    The training step issues ~750 kernels; at static row capacities none of them needs the host, so the whole
    forward + backward — voxeliser, index stream, sparse and dense convolutions, losses, every gradient — is captured
    once and replayed per step.  The host then issues a copy of the batch into the static buffers, one replay, gradient
    clipping and the (fused) optimizer step: the reference's loop (tools/train_utils/train_utils.py:44-56: zero_grad,
    model_func, backward, clip_grad_norm_, optimizer.step) with its first three calls folded into the replay.  Parameter
    gradients live in the graph's memory pool and are rewritten by every replay, so there is no zero_grad between steps.

    points [N, 1+C] (frame index in column 0, frames ascending), gt_boxes [B, M, 8]; N <= max_points, M <= max_gt."""

    def __init__(self, model, batch_size, max_points, max_gt, level_factors=None, warmup=3, example=None):
        assert model.training, "GraphedTrainStep captures the training forward"
        self.model = model
        self.batch_size = int(batch_size)
        self.device = next(model.parameters()).device
        vfe = model.vfe
        c = 1 + vfe.num_point_features
        self.max_points, self.max_gt = int(max_points), int(max_gt)
        self.points = torch.empty((self.max_points, c), dtype=torch.float32, device=self.device)
        self._pad_row = torch.zeros((c,), dtype=torch.float32, device=self.device)
        self._pad_row[0] = self.batch_size - 1
        self._pad_row[1] = float(vfe.point_cloud_range[0]) - 1.0e4          # outside the range: dropped by the voxeliser
        self.points[:] = self._pad_row
        self.gt_boxes = torch.zeros((self.batch_size, self.max_gt, 8), dtype=torch.float32, device=self.device)
        self.static_caps = static_caps_for(model, self.batch_size, self.max_points, training=True,
                                           level_factors=level_factors)
        if example is not None:
            self._load(example[0], example[1])
        s = torch.cuda.Stream(device=self.device)
        s.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(s):
            for _ in range(warmup):                      # allocator pools, workspaces, MIOpen kernel selection
                model.zero_grad(set_to_none=True)
                self._forward_backward()
        torch.cuda.current_stream(self.device).wait_stream(s)
        torch.cuda.synchronize(self.device)
        model.zero_grad(set_to_none=True)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.out = self._forward_backward()

    def _forward_backward(self):
        bd = {'points': self.points, 'gt_boxes': self.gt_boxes, 'batch_size': self.batch_size,
              'static_caps': self.static_caps}
        ret, tb_dict, _disp = self.model(bd)
        loss = ret['loss'].mean()
        loss.backward()
        return {'loss': loss.detach(), 'tb_dict': tb_dict}

    def _load(self, points, gt_boxes):
        n, m = points.shape[0], gt_boxes.shape[1]
        if n > self.max_points or m > self.max_gt or gt_boxes.shape[0] != self.batch_size:
            raise ValueError("batch (%d points, %d boxes) exceeds the captured capacities (%d, %d)"
                             % (n, m, self.max_points, self.max_gt))
        self.points[:n].copy_(points, non_blocking=True)
        if n < self.max_points:
            self.points[n:] = self._pad_row
        self.gt_boxes.zero_()
        self.gt_boxes[:, :m].copy_(gt_boxes, non_blocking=True)

    def __call__(self, points, gt_boxes):
        """Copies the batch in and replays forward + backward; parameter .grad tensors hold the new gradients afterwards.
        Returns the static output dict {'loss', 'tb_dict'} (overwritten by the next call)."""
        self._load(points, gt_boxes)
        self.graph.replay()
        return self.out
