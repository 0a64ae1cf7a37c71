"""Boundary B1 drop-in: the REFERENCE's training-loop function — tools/train_utils/train_utils.py:train_one_epoch — drives OUR
detector through the `pcdet` import alias (tsm-det-pointcloud-_amd/compat/pcdet): `from pcdet.utils import common_utils,
commu_utils` at its top resolves to pcdet_amd, and the model function is our `pcdet.models.model_fn_decorator()` (reference
pcdet/models/__init__.py:40-52: load_data_to_gpu -> model(batch) -> ModelReturn(loss, tb_dict, disp_dict) ->
update_global_step).  tests/golden/ref_dropin.npz holds what that function logged when it ran two iterations on this
detector (tests/golden/make_golden_dropin.py, oracle backend): the frames of each batch and every tb_log.add_scalar.  The
reference source itself is not imported here: the test drives the same two iterations through the same calls —
lr_scheduler.step / zero_grad / model_func / backward / clip_grad_norm_ / optimizer.step, same loader, seeds and numpy
generator state — and checks that the loader yields the same frames and that the same keys are logged with the same values
(no GPU here)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _alias():
    compat = os.path.join(ROOT, "tsm-det-pointcloud-_amd", "compat")
    if compat not in sys.path:
        sys.path.insert(0, compat)
    import pcdet
    return pcdet


def test_pcdet_alias_is_the_same_package():
    pcdet = _alias()
    import pcdet_amd
    import pcdet.models.detectors as a
    import pcdet_amd.models.detectors as b
    from pcdet.models import build_network, load_data_to_gpu, model_fn_decorator      # noqa: F401  (tools/train.py:14-17)
    from pcdet.utils import common_utils, commu_utils
    assert pcdet is pcdet_amd and a is b and a.SECONDNet is b.SECONDNet
    assert sys.modules["pcdet.models.detectors"] is sys.modules["pcdet_amd.models.detectors"]
    assert commu_utils.average_reduce_value(3.0) == 3.0 and commu_utils.get_world_size() == 1
    m = common_utils.AverageMeter()
    m.update(2.0), m.update(4.0)
    assert m.avg == 3.0 and m.val == 4.0


def test_train_loop_reproduces_reference_train_one_epoch_log(monkeypatch):
    """Our detector, optimizer, scheduler and loader through the reference loop's sequence of calls: the loader yields the
    frames the reference's train_one_epoch was handed, and every value it logged comes out again."""
    _alias()
    from oracle.cpu_backend import use_oracle_backend
    import pcdet.models as pm
    from pcdet.config import AttrDict, cfg_from_yaml_file
    from pcdet.datasets import build_dataloader
    from pcdet.utils import commu_utils
    from tools.train_utils.optimization import build_optimizer, build_scheduler
    G = np.load(os.path.join(ROOT, "tests", "golden", "ref_dropin.npz"))
    want = {(str(k), int(i)): float(v) for k, v, i in zip(G["train_log_keys"], G["train_log_values"], G["train_log_iters"])}

    cfg = cfg_from_yaml_file(os.path.join(ROOT, "tsm-det-pointcloud-_amd/tools/cfgs/kitti_models/second.yaml"), AttrDict())
    cfg.DATA_CONFIG.SYNTHETIC_CFG_ID = 0
    ds, loader, _sampler = build_dataloader(cfg.DATA_CONFIG, cfg.CLASS_NAMES, batch_size=2, dist=False, workers=0,
                                            training=True, length=4)
    torch.manual_seed(0)
    model = pm.build_network(cfg.MODEL, len(cfg.CLASS_NAMES), ds)
    optimizer = build_optimizer(model, cfg.OPTIMIZATION)
    sched, _ = build_scheduler(optimizer, total_iters_each_epoch=2, total_epochs=1, last_epoch=-1, optim_cfg=cfg.OPTIMIZATION)
    # no GPU in this container: load_data_to_gpu targets the host, sparse ops run on the oracle backend
    monkeypatch.setattr(pm, "load_data_to_gpu", functools.partial(pm.load_data_to_gpu, device=torch.device("cpu")))
    model_func = pm.model_fn_decorator()
    before = {k: v.detach().clone() for k, v in model.named_parameters()}
    seen = {}

    it = 0
    iter(loader)                       # the iterator the caller hands in; an epoch over the whole loader starts a fresh one
    batches = iter(loader)
    np.random.seed(0)                  # the training-mode point shuffle of the data processor draws from numpy's generator
    with use_oracle_backend():
        for frames in G["train_frames"]:
            batch = next(batches)
            assert [int(f) for f in batch["frame_id"]] == [int(f) for f in frames]    # the reference loop's batches
            sched.step(it)
            lr = optimizer.param_groups[0]["lr"]
            seen[("meta_data/learning_rate", it)] = lr
            model.train()
            optimizer.zero_grad()
            batch["accumulated_iter"] = it
            loss, tb_dict, disp_dict = model_func(model, batch)
            loss.backward()
            torch.nn.utils.clip_grad_norm_(model.parameters(), cfg.OPTIMIZATION.GRAD_NORM_CLIP)
            optimizer.step()
            it += 1
            assert isinstance(disp_dict, dict) and commu_utils.average_reduce_value(1.5) == 1.5
            seen[("train/loss", it)] = float(loss.detach())
            seen[("meta_data/learning_rate", it)] = lr
            for k, v in tb_dict.items():
                seen[("train/" + k, it)] = float(v)
    assert it == 2 and int(model.global_step) == 2            # update_global_step ran inside model_func
    assert sorted(seen) == sorted(want)
    for (key, i), v in want.items():
        # iteration 1 runs on the initial weights and the learning rates are schedule values: to float32 rounding.  After
        # the first AdamW step (~lr * sign(grad) per weight) the CPU's rounding of near-zero gradients (thread count, ISA)
        # moves iteration 2's losses by ~0.1 %; a missing or wrong update moves them several-fold (2.65 -> 8.5 here).
        rel = 1e-5 if i <= 1 or key == "meta_data/learning_rate" else 2e-2
        assert seen[(key, i)] == pytest.approx(v, rel=rel, abs=1e-6), (key, i)
    assert all(np.isfinite(v) for v in seen.values())
    assert {"train/rpn_loss_cls", "train/rpn_loss_loc", "train/rpn_loss_dir"} <= {k for k, _i in seen}
    moved = [k for k, v in model.named_parameters() if not torch.equal(v, before[k])]
    assert any(k.startswith("backbone_3d.conv_input.0") for k in moved) and any(k.startswith("dense_head") for k in moved)
    assert model.training
