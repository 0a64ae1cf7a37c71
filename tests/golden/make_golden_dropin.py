"""Generate tests/golden/ref_dropin.npz: what the REFERENCE's own model and training-loop sources compute when they run
on this package's operators (the `spconv` / `pcdet` alias packages in tsm-det-pointcloud-_amd/compat), sparse ops on the
CPU oracle backend.  tests/test_dropin_reference_*.py check this package's own modules against these vectors.

Captured, per scenario (same seeds and inputs as the tests):
  bb8x_*   VoxelBackBone8x + HeightCompression (reference spconv_backbone.py / height_compression.py), 2 frames of cfg 0:
           state_dict keys and shapes, x_conv1..4 indices + features, spatial_features;
  res_*    VoxelResBackBone8x, 1 frame: state_dict keys, x_conv1..4 + encoded features;
  unet_*   UNetV2 (reference spconv_unet.py), 1 frame: state_dict keys and shapes, point_features, raw_points_bxyz,
           encoded indices + features;
  train_*  two iterations of the reference's tools/train_utils/train_utils.py:train_one_epoch driving SECONDNet through
           model_fn_decorator: the frame ids of every batch and every tb_log.add_scalar(key, value, iter) it made.
Float arrays above 8192 elements are stored as 128 whole rows picked by a generator seeded from the name (`<name>_rowidx`,
`<name>_rows`), EVERY row projected in float64 on two fixed random directions (`<name>_proj` = rows @ `<name>_projmat`),
their float64 column sums (`<name>_colsum`) and shape (`<name>_shape`); spatial_features as [B*H*W, C] pixel rows.  Only DATA is written; no reference source or bytecode.  The reference modules load THIS package's
weights (same seeds as the tests), so the vectors pin "reference source on our operators == our modules".

Run:  python tests/golden/make_golden_dropin.py <path to a checkout of the reference repository>
"""
import functools
import importlib
import importlib.util
import os
import sys
import types
import zlib

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
PKG = os.path.join(ROOT, "tsm-det-pointcloud-_amd")
for _p in (ROOT, PKG, os.path.join(PKG, "compat")):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def _ref_packages(ref, names):
    """Namespaces for reference packages without running their __init__; returns the pcdet modules they replaced."""
    saved = {k: v for k, v in sys.modules.items() if k == "pcdet" or k.startswith("pcdet.")}
    for k in saved:
        del sys.modules[k]
    for n in names:
        m = types.ModuleType(n)
        m.__path__ = [os.path.join(ref, *n.split("."))]
        sys.modules[n] = m
    return saved


def _restore(saved):
    for k in [k for k in sys.modules if k == "pcdet" or k.startswith("pcdet.")]:
        del sys.modules[k]
    sys.modules.update(saved)


def import_reference_modules(ref):
    import spconv.pytorch  # noqa: F401  (our alias)
    sys.modules.setdefault("SharedArray", types.ModuleType("SharedArray"))
    saved = _ref_packages(ref, ("pcdet", "pcdet.utils", "pcdet.models", "pcdet.models.backbones_3d",
                                "pcdet.models.backbones_2d", "pcdet.models.backbones_2d.map_to_bev"))
    try:
        bb = importlib.import_module("pcdet.models.backbones_3d.spconv_backbone")
        hc = importlib.import_module("pcdet.models.backbones_2d.map_to_bev.height_compression")
        unet = importlib.import_module("pcdet.models.backbones_3d.spconv_unet")
    finally:
        _restore(saved)
    return bb, hc, unet


def _put(out, name, a):
    """Whole, or (large float arrays) a seeded row sample + float64 column sums + shape."""
    a = np.asarray(a)
    if a.dtype.kind != "f" or a.size <= 8192:
        out[name] = a
        return
    rows = a.reshape(a.shape[0], -1)
    idx = np.sort(np.random.default_rng(zlib.crc32(name.encode())).choice(rows.shape[0], 128, replace=False))
    out[name + "_shape"] = np.array(a.shape, np.int64)
    out[name + "_rowidx"] = idx.astype(np.int64)
    out[name + "_rows"] = rows[idx]
    out[name + "_colsum"] = rows.astype(np.float64).sum(0)
    r = np.random.default_rng(zlib.crc32(name.encode()) + 1).standard_normal((rows.shape[1], 2))
    out[name + "_projmat"] = r
    out[name + "_proj"] = rows.astype(np.float64) @ r                 # every row, through two fixed random directions


def _keys_shapes(prefix, sd, out):
    out[prefix + "keys"] = np.array(list(sd.keys()))
    out[prefix + "shapes"] = np.array(["x".join(str(s) for s in v.shape) for v in sd.values()])


def _vox(ds, b, bsz):
    from spx import ops
    vox = ops.voxelize(torch.from_numpy(b["points"]), ds.point_cloud_range, ds.voxel_size, 5, 16000, batch_size=bsz,
                       batch_col=0, xyz_col=1, feat_col=1, want_voxels=False)
    return {"voxel_features": vox["mean"], "voxel_coords": vox["coords"].float(), "batch_size": bsz}


def backbones(ref, out):
    from oracle.cpu_backend import use_oracle_backend
    from pcdet_amd.config import AttrDict
    from pcdet_amd.datasets import SyntheticDataset
    from pcdet_amd.models.backbones_3d import UNetV2, VoxelBackBone8x, VoxelResBackBone8x
    ref_bb, ref_hc, ref_unet = import_reference_modules(ref)
    ds = SyntheticDataset(cfg_id=0)

    torch.manual_seed(0)
    ours = VoxelBackBone8x(AttrDict(), 4, ds.grid_size)
    theirs = ref_bb.VoxelBackBone8x(AttrDict(), 4, ds.grid_size)
    theirs.load_state_dict(ours.state_dict())
    theirs.eval()
    _keys_shapes("bb8x_", theirs.state_dict(), out)
    with torch.no_grad(), use_oracle_backend():
        t = ref_hc.HeightCompression(AttrDict(NUM_BEV_FEATURES=256))(theirs(_vox(ds, ds.collate_batch([ds[0], ds[1]]), 2)))
    for k in ("x_conv1", "x_conv2", "x_conv3", "x_conv4"):
        out["bb8x_%s_indices" % k] = t["multi_scale_3d_features"][k].indices.numpy()
        _put(out, "bb8x_%s_features" % k, t["multi_scale_3d_features"][k].features.numpy())
    sf = t["spatial_features"].numpy()
    _put(out, "bb8x_spatial_features", sf.transpose(0, 2, 3, 1).reshape(-1, sf.shape[1]))      # pixel rows
    out["bb8x_spatial_shape"] = np.array(sf.shape, np.int64)
    out["bb8x_stride"] = np.array(t["encoded_spconv_tensor_stride"])

    torch.manual_seed(1)
    ours = VoxelResBackBone8x(AttrDict(), 4, ds.grid_size)
    theirs = ref_bb.VoxelResBackBone8x(AttrDict(), 4, ds.grid_size)
    theirs.load_state_dict(ours.state_dict())
    theirs.eval()
    out["res_keys"] = np.array(list(theirs.state_dict().keys()))
    with torch.no_grad(), use_oracle_backend():
        t = theirs(_vox(ds, ds.collate_batch([ds[0]]), 1))
    for k in ("x_conv1", "x_conv2", "x_conv3", "x_conv4"):
        _put(out, "res_%s_features" % k, t["multi_scale_3d_features"][k].features.numpy())
    _put(out, "res_encoded_features", t["encoded_spconv_tensor"].features.numpy())

    torch.manual_seed(2)
    kw = dict(voxel_size=ds.voxel_size, point_cloud_range=ds.point_cloud_range)
    ours = UNetV2(AttrDict(), 4, ds.grid_size, **kw)
    theirs = ref_unet.UNetV2(AttrDict(), 4, np.asarray(ds.grid_size), **kw)   # the reference adds [1, 0, 0] to an ndarray
    theirs.load_state_dict(ours.state_dict())
    theirs.eval()
    _keys_shapes("unet_", theirs.state_dict(), out)
    with torch.no_grad(), use_oracle_backend():
        t = theirs(_vox(ds, ds.collate_batch([ds[0]]), 1))
    _put(out, "unet_point_features", t["point_features"].numpy())
    _put(out, "unet_raw_points_bxyz", t["raw_points_bxyz"].numpy())
    out["unet_encoded_indices"] = t["encoded_spconv_tensor"].indices.numpy()
    _put(out, "unet_encoded_features", t["encoded_spconv_tensor"].features.numpy())


def train_loop(ref, out):
    import tqdm
    import pcdet  # noqa: F401  (our alias package: the reference's `from pcdet.utils import ...` resolves to pcdet_amd)
    import pcdet.models as pm
    from oracle.cpu_backend import use_oracle_backend
    from pcdet.config import AttrDict, cfg_from_yaml_file
    from pcdet.datasets import build_dataloader
    from tools.train_utils.optimization import build_optimizer, build_scheduler
    spec = importlib.util.spec_from_file_location("ref_train_utils", os.path.join(ref, "tools/train_utils/train_utils.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)

    cfg = cfg_from_yaml_file(os.path.join(PKG, "tools/cfgs/kitti_models/second.yaml"), AttrDict())
    cfg.DATA_CONFIG.SYNTHETIC_CFG_ID = 0
    ds, loader, _sampler = build_dataloader(cfg.DATA_CONFIG, cfg.CLASS_NAMES, batch_size=2, dist=False, workers=0,
                                            training=True, length=4)
    torch.manual_seed(0)
    model = pm.build_network(cfg.MODEL, len(cfg.CLASS_NAMES), ds)
    optimizer = build_optimizer(model, cfg.OPTIMIZATION)
    sched, _ = build_scheduler(optimizer, total_iters_each_epoch=2, total_epochs=1, last_epoch=-1, optim_cfg=cfg.OPTIMIZATION)
    inner = pm.model_fn_decorator()
    frames = []

    def model_func(model, batch):
        frames.append([int(f) for f in batch["frame_id"]])
        return inner(model, batch)

    load = functools.partial(pm.load_data_to_gpu, device=torch.device("cpu"))
    pm.load_data_to_gpu, saved_load = load, pm.load_data_to_gpu
    seen = []

    class _Tb(object):
        def add_scalar(self, key, val, it):
            seen.append((key, float(val), it))

    np.random.seed(0)                  # the training-mode point shuffle of the data processor draws from numpy's generator
    try:
        with use_oracle_backend(), tqdm.trange(0, 1, desc="epochs", disable=True) as tbar:
            it = mod.train_one_epoch(model, optimizer, loader, model_func, lr_scheduler=sched, accumulated_iter=0,
                                     optim_cfg=cfg.OPTIMIZATION, rank=0, tbar=tbar, total_it_each_epoch=len(loader),
                                     dataloader_iter=iter(loader), tb_log=_Tb())
    finally:
        pm.load_data_to_gpu = saved_load
    assert it == 2 and int(model.global_step) == 2
    out["train_frames"] = np.array(frames, np.int64)
    out["train_log_keys"] = np.array([k for k, _v, _i in seen])
    out["train_log_values"] = np.array([v for _k, v, _i in seen], np.float64)
    out["train_log_iters"] = np.array([i for _k, _v, i in seen], np.int64)


def main():
    if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "pcdet")):
        sys.exit("usage: python tests/golden/make_golden_dropin.py <reference checkout>")
    ref = os.path.abspath(sys.argv[1])
    import __graft_entry__ as ge
    ge.build(verbose=False)
    out = {}
    backbones(ref, out)
    train_loop(ref, out)
    path = os.path.join(HERE, "ref_dropin.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
