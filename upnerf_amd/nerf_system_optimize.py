"""Test-time optimisation (TTO) on the HIP path: the callers of render_rays in models/nerf_system_optmize.py
(forward 84-111, training_step 113-150, validation_step 152-188) for ONE held-out image -- frozen NeRF weights, a
fresh appearance embedding and (pose stage) the image's se(3) refinement are optimised against the colour loss.

`eval_train_poses` and `tto_from_checkpoint` are the two things eval.py / tto.py do with a trained checkpoint before
rendering: the pose error of the training cameras after Sim(3) alignment (eval.py:13-42) and a TTO system whose fields
come from the checkpoint and whose held-out cameras start from the aligned ground truth
(nerf_system_optmize.py:254-317); the pose algebra is in pose_align.py.

Differences by design: the reference leaves the NeRF weights trainable-but-unused (it computes and discards all
weight gradients); here they are frozen, so the backward pass skips every weight-gradient
kernel.

Metrics: validation reports PSNR and, when the batch carries `img_wh`, SSIM (metrics.py: a HIP kernel on the device-resident
render, where the reference copies every render to the host for kornia).  LPIPS (AlexNet) is reported as well once a
`metrics.LpipsAlex` built from the user's weight files is attached as `system.lpips_model` (lpips.py; None by default, and
then every dictionary and file is what it is without it).  `best` records the epoch of the highest PSNR as the reference
does; `write_nvs_results` / `read_nvs_results` are its psnr.pkl / ssim.pkl / lpips.pkl bookkeeping and what eval.py prints
from it.  Unlike Lightning, run_stage has no sanity validation
before the first epoch (tto.py:63, 87), so `best` never holds the starting PSNR."""
from __future__ import annotations

import torch
from torch import nn

from . import zero_pool
from .camera import refine_and_get_rays
from .losses import _const
from .metrics import lpips_rays, ssim_rays
from .nerf_system import NeRFSystem
from .ops import EMBED_PREFETCH, embed_rows
from .optim import get_optimizer
from .rendering import join_rays, render_rays


class NeRFSystemOptimize(NeRFSystem):
    supports_graph_step = True  # the step splits like NeRFSystem's (graph_step.py): one graph replay per TTO step
    lpips_model = None  # a metrics.LpipsAlex: validation then reports LPIPS too (a plain attribute: not in state_dict)

    def __init__(self, hparams, train_dataset=None, val_dataset=None, pose_optimize=True):
        super().__init__(hparams, train_dataset, val_dataset)
        self.pose_optimize = pose_optimize
        # only s_rgb_fine is ever read here, so the coarse field stops at its density head (set False to get the
        # reference's full set of coarse maps back)
        self.coarse_sigma_only = True
        # the best validation epoch (nerf_system_optmize.py:22-23): psnr, ssim, step and the stage's trainable rows
        self.best = {"psnr": 0.0, "ssim": None, "step": None}

    def dataset_setup(self):
        """models/nerf_system_optmize.py:233-252: the held-out image `optimize_num` of hparams["dataset_name"]'s
        `_optimize` dataset, the whole image (pose stage) or its left / right half (appearance stage)."""
        from .datasets import dataset_dict
        hp = self.hparams
        dataset = dataset_dict.get(f"{hp.get('dataset_name')}_optimize")
        if dataset is None:
            return super().dataset_setup()  # raises NotImplementedError
        kw = dict(root_dir=hp["root_dir"], scene_name=hp["scene_name"], img_downscale=hp["phototourism.img_downscale"],
                  use_cache=hp.get("phototourism.use_cache", False), near=hp["nerf.near"], far=hp["nerf.far"],
                  pose_optimize=hp.get("pose_optimize", self.pose_optimize), optimize_num=hp["optimize_num"],
                  device=self.dataset_device)
        self.train_dataset = dataset(split="train", camera_noise=hp["pose.noise"], **kw)
        self.val_dataset = dataset(split="val", camera_noise=hp["pose.noise"], **kw)

    def model_setup(self, trained_state=None, n_test_images: int = None):
        if n_test_images is None:  # the reference sizes the test tables by N_images_test (line 257); 1 without a scene
            n_test_images = getattr(self.train_dataset, "N_images_test", None) or 1
        super().model_setup()
        if trained_state is not None:
            self.load_state_dict(trained_state, strict=False)
        hp = self.hparams
        # only trainable appearance table: one row per test image (nerf_system_optmize.py:254-256)
        self.embedding_fine_a = nn.Embedding(n_test_images, hp["nerf.appearance_dim"])
        self.embeddings["fine_a"] = self.embedding_fine_a
        self.se3_refine = nn.Embedding(n_test_images, 6)
        nn.init.zeros_(self.se3_refine.weight)
        for m in (self.nerf_coarse, self.nerf_fine):
            m.encode_candidate = False  # nerf_system_optmize.py:265-266
            for p in m.parameters():
                p.requires_grad_(False)
        for k in ("coarse_a", "coarse_c", "fine_c"):
            if k in self.embeddings:
                self.embeddings[k].weight.requires_grad_(False)
        self.set_progress(1.0)  # all encoding bands on, schedule finished

    def configure_optimizers(self):
        if self.pose_optimize:  # nerf_system_optmize.py:48-58
            opts = [get_optimizer("adam", 5e-3, [self.embedding_fine_a]), get_optimizer("adam", 1e-4, [self.se3_refine])]
        else:  # appearance stage: AdamW(1e-1) (lines 59-64); capturable: its step counter lives on the device, so the update
            # can sit inside the replayed graph (same update rule; on a CPU system the flag is not available)
            on_gpu = self.embedding_fine_a.weight.is_cuda
            opts = [torch.optim.AdamW(self.embedding_fine_a.parameters(), lr=1e-1, **({"capturable": True} if on_gpu else {}))]
        scheds = [{"scheduler": torch.optim.lr_scheduler.ConstantLR(o, factor=1.0, total_iters=0), "interval": "step"}
                  for o in opts]
        return opts, scheds

    def forward(self, rays, img_idx, train=True, u_list=None):
        hp = self.hparams
        chunk = rays.shape[0] if train else hp["val.chunk_size"]
        outs = []
        for i in range(0, rays.shape[0], chunk):
            outs.append(render_rays(models=self.models, embeddings=self.embeddings,
                                    rays=rays if chunk >= rays.shape[0] else rays[i:i + chunk],
                                    img_idx=img_idx[i:i + chunk], sched_mult=1.0, N_samples=hp["nerf.N_samples"],
                                    use_disp=hp["nerf.use_disp"], perturb=hp["nerf.perturb"] if train else 0,
                                    N_importance=hp["nerf.N_importance"], encode_feat=hp["nerf.feat_dim"] > 0, u_list=u_list,
                                    coarse_sigma_only=self.coarse_sigma_only))
        return {k: (outs[0][k] if len(outs) == 1 else torch.cat([o[k] for o in outs], 0)) for k in outs[0]}

    def rays_from_batch(self, batch):
        se3 = embed_rows(self.se3_refine, batch["img_idx"], defer_grad=True) if self.pose_optimize else None
        o, d = refine_and_get_rays(se3, batch["c2w"], batch["directions"])
        return join_rays(o, d, batch["ray_infos"])

    def compute_loss(self, batch, u_list=None):
        rays = self.rays_from_batch(batch)
        self._last_rays = rays  # kept for tests (gradient w.r.t. the rays), as NeRFSystem.compute_loss does
        res = self(rays, batch["img_idx"], u_list=u_list)
        loss = ((res["s_rgb_fine"] - batch["rgbs"]) ** 2).mean()  # nerf_system_optmize.py:129
        return loss, {"rgb": loss}, res

    # the three pieces of a step (NeRFSystem.training_step composes them; graph_step.GraphedTrainingStep captures the first two)
    def _step_backward(self, batch, u_list=None):
        with zero_pool.step(batch["img_idx"].device), EMBED_PREFETCH.scope(self._per_image_tables()):
            loss, loss_d, _ = self.compute_loss(batch, u_list=u_list)
            for o in self._opts_scheds()[0]:
                o.zero_grad()
            self.manual_backward(loss, gradient=_const(1.0, loss.device))
        return loss, loss_d

    def _step_host(self, loss, loss_d, done):
        opts, _ = self._opts_scheds()
        for o, runs in zip(opts, done):
            if runs is not None:
                o.step_host(runs)
        self.global_step += len(opts)

    def training_step(self, batch, batch_nb=0, u_list=None):
        loss, loss_d = self._step_backward(batch, u_list=u_list)
        self._step_host(loss, loss_d, self._step_update())
        return loss

    @torch.no_grad()
    def validation_step(self, batch, batch_nb=0):
        """Full-image render in val.chunk_size chunks, perturb = 0; returns the PSNR on s_rgb_fine, and its SSIM when the
        batch carries the image size `img_wh` (W, H) as the reference's validation batches do (lines 174-183); with a
        `lpips_model` attached, its LPIPS as well (line 184)."""
        res = self(self.rays_from_batch(batch), batch["img_idx"], train=False)
        mse = ((res["s_rgb_fine"] - batch["rgbs"]) ** 2).mean()
        out = {"val_psnr": -10.0 * torch.log10(mse), "s_rgb_fine": res["s_rgb_fine"], "s_depth_fine": res["s_depth_fine"]}
        if batch.get("img_wh") is not None:
            rgbs = batch["rgbs"].reshape(res["s_rgb_fine"].shape)
            out["val_ssim"] = ssim_rays(res["s_rgb_fine"], rgbs, batch["img_wh"]).reshape(())
            if self.lpips_model is not None:
                out["val_lpips"] = lpips_rays(self.lpips_model, res["s_rgb_fine"], rgbs, batch["img_wh"]).reshape(())
        return out

    def validation_epoch_end(self, outputs):
        """Mean PSNR (and SSIM / LPIPS, over the outputs that carry them) of the validation images (nerf_system_optmize.py:190-196),
        and the record of the best epoch in `self.best` (lines 195-198)."""
        if not outputs:
            return None
        out = {"val/psnr": torch.stack([x["val_psnr"].reshape(()) for x in outputs]).mean()}
        ss = [x["val_ssim"].reshape(()) for x in outputs if "val_ssim" in x]
        if ss:
            out["val/ssim"] = torch.stack(ss).mean()
        ls = [x["val_lpips"].reshape(()) for x in outputs if "val_lpips" in x]
        if ls:
            out["val/lpips"] = torch.stack(ls).mean()
        for k, v in out.items():
            self.log(k, v)
        self._update_best(out)
        return out

    def _update_best(self, metrics):
        """Replace `self.best` on a strictly greater val/psnr: that epoch's PSNR and SSIM (and LPIPS, when it was computed), the
        step, and copies of the stage's trainable rows (the reference saves them as best_pose_NN.npy)."""
        psnr = metrics["val/psnr"]
        if not float(psnr) > float(self.best["psnr"]):  # (a NaN never replaces it)
            return
        ssim = metrics.get("val/ssim")
        best = {"psnr": psnr.detach().clone(), "ssim": None if ssim is None else ssim.detach().clone(),
                "step": int(self.global_step), "embedding_fine_a": self.embedding_fine_a.weight.detach().clone()}
        if self.pose_optimize:
            best["se3_refine"] = self.se3_refine.weight.detach().clone()
        if "val/lpips" in metrics:
            best["lpips"] = metrics["val/lpips"].detach().clone()
        self.best = best


def run_stage(system: NeRFSystemOptimize, train_batches, n_batches_per_epoch: int, max_epochs: int, val_batches=(),
              graph: bool = True, image_sink=None):
    """One test-time-optimisation stage the way tto.py:56-91 runs it: `max_epochs` passes over the held-out image's rays
    (50 for the pose stage, 20 for the appearance stage), a validation render after every epoch, no checkpoints.
    Returns the Trainer (its `history` holds val/psnr per epoch, and val/ssim when the validation batches carry img_wh);
    `system.best` holds the epoch with the highest PSNR.  image_sink (e.g. visualization.ImageWriter): receives `GT` and
    `rgb_fine` of every validation render under the tag `val_<optimize_num>` (nerf_system_optmize.py:190-193); without one,
    the sink `tto_from_checkpoint` was given, if any."""
    from .trainer import Trainer
    if image_sink is None:
        image_sink = getattr(system, "image_sink", None)
    opts = system.optimizers()
    n_opt = len(opts) if isinstance(opts, (list, tuple)) else 1
    budget = int(system.global_step) + max_epochs * n_batches_per_epoch * n_opt
    return Trainer(budget, val_check_interval=1.0, dirpath=None, graph=graph, image_sink=image_sink).fit(
        system, train_batches, n_batches_per_epoch, val_batches)


def write_nvs_results(dirpath: str, optimize_num: int, best: dict) -> None:
    """nerf_system_optmize.py:208-228: merge the best PSNR and SSIM of held-out image `optimize_num` into
    `<dirpath>/psnr.pkl` and `ssim.pkl` ({image number: 0-d CPU tensor}, the files eval.py reads), and its LPIPS into
    `lpips.pkl` when `best` holds one (a system with a `lpips_model`); no lpips.pkl otherwise."""
    import os
    import pickle
    os.makedirs(dirpath, exist_ok=True)
    for name in ("psnr", "ssim", "lpips"):
        if best.get(name) is None:
            continue
        path = os.path.join(dirpath, f"{name}.pkl")
        table = {}
        if os.path.isfile(path):
            with open(path, "rb") as f:
                table = pickle.load(f)
        table[int(optimize_num)] = torch.as_tensor(best[name]).detach().reshape(()).cpu()
        with open(path, "wb") as f:
            pickle.dump(table, f)


def read_nvs_results(dirpath: str) -> dict:
    """eval.py:48-79: the mean PSNR, SSIM and LPIPS over the held-out images in `dirpath` (None where a file is absent, as
    lpips.pkl is for a run without a `lpips_model`; a directory the reference wrote reads too)."""
    import os
    import pickle
    out = {"psnr": None, "ssim": None, "lpips": None}
    for name in ("psnr", "ssim", "lpips"):
        path = os.path.join(dirpath, f"{name}.pkl")
        if os.path.isfile(path):
            with open(path, "rb") as f:
                vals = [float(v) for v in pickle.load(f).values()]
            out[name] = sum(vals) / len(vals) if vals else None
    return out


def eval_train_poses(checkpoint, noised_poses, gt_poses, device="cuda") -> dict:
    """eval.py:13-42: trained se(3) refinements composed with the (noised) training poses, Sim(3)-aligned to the ground
    truth; mean rotation error in degrees and mean translation error, as eval.py prints them, plus the per-image values."""
    import math
    from .checkpoint import read_checkpoint
    from .pose_align import pose_metric, refined_poses
    se3 = read_checkpoint(checkpoint)["state_dict"]["se3_refine.weight"]
    refined = refined_poses(se3.to(device), noised_poses.to(device)).cpu()
    err, aligned, gt = pose_metric(refined, gt_poses)
    if err is None:
        return {"train/pose_R": None, "train/pose_t": None, "refined": refined, "aligned": aligned}
    return {"train/pose_R": float(err["R"].mean()) * 180.0 / math.pi, "train/pose_t": float(err["t"].mean()),
            "R": err["R"], "t": err["t"], "refined": refined, "aligned": aligned}


def tto_from_checkpoint(checkpoint, pose_optimize: bool, n_test_images: int = 1, gt_train_poses=None, gt_test_poses=None,
                        device="cuda", image_sink=None, lpips=None, **overrides):
    """NeRFSystemOptimize for the held-out images of a trained run (nerf_system_optmize.py:254-317): hyper-parameters and
    fields from the checkpoint, a fresh appearance row per test image and, when ground-truth poses are given, their
    initial cameras in the frame the model was trained in.  Returns (system, initial test poses or None).
    image_sink: kept on the system (`system.image_sink`) for the stages `run_stage` runs on it.  lpips: a metrics.LpipsAlex
    (moved to `device`), kept as `system.lpips_model`: validation then reports LPIPS as well."""
    from .checkpoint import read_checkpoint
    from .pose_align import init_test_poses, refined_poses
    ck = read_checkpoint(checkpoint)
    hp = dict(ck["hyper_parameters"])
    hp.update(overrides)
    sd = ck["state_dict"]
    n_train = sd["se3_refine.weight"].shape[0] if "se3_refine.weight" in sd else sd["embedding_fine_a.weight"].shape[0]
    from .nerf_system import SyntheticDataset
    system = NeRFSystemOptimize(hp, SyntheticDataset(n_train), pose_optimize=pose_optimize)
    keep = {k: v for k, v in sd.items() if not k.startswith(("embedding_fine_a.", "se3_refine."))}
    system.model_setup(trained_state=keep, n_test_images=n_test_images)
    system.to(device)
    system.image_sink = image_sink
    if lpips is not None:
        system.lpips_model = lpips.to(device)
    init = None
    if gt_train_poses is not None and gt_test_poses is not None:
        ident = torch.eye(3, 4).repeat(n_train, 1, 1)  # line 286: the trained refinements over identity poses
        init = init_test_poses(refined_poses(sd["se3_refine.weight"].to(device), ident.to(device)).cpu(),
                               gt_train_poses, gt_test_poses)
    return system, init
