"""Mirror of the fitting API of the reference's optimize_sequence.py: init_params (:181-250), get_optimizers (:253-310) and
optimize_hand_sequence (:313-816, loop body :446-582).  What looks at a fit — mirror_render and the post-fit evaluation evaluate_sequence
(:595-816) — lives in harp_amd/evaluate.py and get_mesh_subdivider (:67-89) in utils/visualize.py; all three are re-exported here.

`optimize_hand_sequence` keeps the reference's signature and schedule (stages, batch 18, shuffle, dense Adam groups and
learning rates, ReduceLROnPlateau(patience=40) on the coarse group, checkpoint format) but runs every step through the fused
engine (harp_amd/engine.py) on HBM-resident targets.  The per-op API (`prepare_mesh`, `render_image`, losses) stays available
for callers that drive autograd themselves (`visualize_val`-style code)."""
import contextlib

import numpy as np
import torch

from .engine import FitEngine, LOSS_NAMES
from .evaluate import EVAL_CHUNK, evaluate_sequence, mirror_render  # noqa: F401  (re-export: the post-fit evaluation lives in evaluate.py)
from .synth import build_topology
from .utils import file_utils
from .utils.data_util import ResidentTargets
from .utils.visualize import get_mesh_subdivider, params_on  # noqa: F401  (re-export: get_mesh_subdivider, :67-89)


def load_uv_mask(configs, uv_size):
    """optimize_sequence.py:174-178"""
    from PIL import Image
    uv_mask_pil = Image.open(configs["uv_mask"]).convert("L").resize(uv_size)
    return torch.tensor(np.asarray(uv_mask_pil) / 255)


def init_params(input_params, VERT_DISPS, VERT_DISPS_NORMALS, VERTS_COLOR, mano_faces, verts_textures, VERTS_UVS=None, FACES_UVS=None,
                model_type="harp", use_arm=False, configs=None, device="cuda", uv_mask=None):
    """optimize_sequence.py:181-250: the same dict (keys, shapes, initial values).  All leaves live on `device` (the reference keeps
    most of them on the CPU and copies them every iteration)."""
    if model_type != "harp" or verts_textures:
        raise NotImplementedError("model_type 'harp' with UV textures is the path in scope (SURVEY.md §8)")
    P = lambda t: torch.nn.Parameter(t.detach().clone().float().to(device), requires_grad=True)
    params = {}
    params["trans"], params["pose"], params["rot"] = P(input_params["trans"]), P(input_params["pose"]), P(input_params["rot"])
    params["shape"] = P(input_params["shape"].mean(dim=0))
    params["wrist_pose"] = P(torch.zeros([params["pose"].shape[0], 3]))
    params["init_joints"] = input_params["joints"]
    n_mesh_verts = 4083 if use_arm else 3093
    params["verts_disps"] = P(torch.zeros(n_mesh_verts, 1 if (VERT_DISPS_NORMALS or not VERT_DISPS) else 3))
    verts_rgb_init = torch.from_numpy(VERTS_COLOR) if VERTS_COLOR is not None else torch.ones(778, 3)
    params["verts_rgb"] = P(verts_rgb_init)
    params["verts_uvs"], params["faces_uvs"] = VERTS_UVS, FACES_UVS
    params["texture"] = P(torch.tensor([232, 190, 172]).repeat(1, 512, 512, 1) / 255.)
    params["uv_mask"] = uv_mask if uv_mask is not None else load_uv_mask(configs, params["texture"].shape[1:3])
    params["normal_map"] = P(torch.tensor([0.0, 0.0, 1.0]).repeat(1, 512, 512, 1))
    total_frame = input_params["cam"].shape[0]
    params["light_positions"] = P(torch.tensor(((-0.5, -0.5, -0.5),)).repeat(total_frame, 1))
    params["amb_ratio"] = P(torch.tensor(0.4))
    params["mesh_faces"] = mano_faces
    params["cam"] = P(input_params["cam"])
    return params


def get_optimizers(params, configs):
    """optimize_sequence.py:253-310 (torch optimisers over the parameter dict, for callers using the autograd API)."""
    pose_params = [params["pose"], params["cam"]]
    shape_params = [params["verts_disps"], params["shape"]] if configs["use_vert_disp"] else [params["shape"]]
    groups = [{"params": pose_params, "lr": 1.0e-3}]
    if configs["use_arm"] and configs["opt_arm_pose"]:
        groups.append({"params": [params["wrist_pose"], params["rot"]], "lr": 1.0e-3})
    if not configs["known_appearance"]:
        groups.append({"params": shape_params, "lr": 1.0e-3})
    opt_coarse = torch.optim.Adam(groups)
    app = [params["light_positions"], params["amb_ratio"]]
    if not configs["known_appearance"]:
        app += [params["texture"], params["normal_map"]]
    opt_app = torch.optim.Adam(app, lr=1.0e-2)
    sched_coarse = torch.optim.lr_scheduler.ReduceLROnPlateau(opt_coarse, patience=40)
    return opt_coarse, opt_app, sched_coarse


def show_img_pair(ypred_np, ytrue_np, step=-1, silhouette=False, save_img_dir=None, prefix="", max_side=1024, sheet_hook=None):
    """optimize_sequence.py:37-64 as one 3 x 3 uint8 contact sheet made on the device (ops.sheet_u8; cells edge to edge, box-averaged by
    harp_amd.monitor.box_factor): the first 9 frames of `ypred_np`, or with silhouette=True the overlay (true mask, 0, predicted mask).
    Takes HIP tensors; numpy arrays and CPU tensors are uploaded.  Writes save_img_dir + prefix + ["sil_"] + "%04d.jpg" % step, or with
    save_img_dir=None returns the (H,W,3) uint8 numpy sheet instead of opening a window.  sheet_hook(name, u8, sources) sees the sheet
    and the float tensors it was made from."""
    from . import monitor, ops
    up = lambda x: (x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x))).detach().to(device="cuda", dtype=torch.float32)[:9]
    ypred = up(ypred_np)
    d = monitor.box_factor(max(ypred.shape[1:3]), max_side)
    if silhouette:
        ytrue = up(ytrue_np)
        sheet, sources = ops.sheet_u8(ytrue, ypred, mode="overlay", d=d), {"y_sil_true": ytrue, "y_sil_pred": ypred}
    else:
        sheet, sources = ops.sheet_u8(ypred, mode="image", d=d), {"y_pred": ypred}
    u8 = sheet.cpu().numpy()
    name = prefix + ("sil_" if silhouette else "") + "%04d.jpg" % step
    if sheet_hook is not None:
        sheet_hook(name, u8, sources)
    if save_img_dir is None:
        return u8
    monitor.encode_jpeg(save_img_dir + name, u8)


def visualize_val(val_images_dataloader, epoch_id, device, params, val_params, configs, hand_layer, mesh_subdivider, opt_app=None,
                  use_verts_textures=False, GLOBAL_POSE=False, SHARED_TEXTURE=True, sheet_hook=None):
    """optimize_sequence.py:97-171 for callers that drive their own loop: the first batch of `val_images_dataloader` rendered under
    torch.no_grad() with the fit's shape, pose, displacements, texture, normal map and light and the validation sequence's own cam, trans
    and rot (harp_amd.monitor.merge_val_params; `val_params` itself is left as it is), written as val_%04d.jpg; the atlas as uv_%04d.jpg
    and normal_%04d.jpg under configs["base_output_dir"].  In scope: UV textures, one shared texture, no global pose."""
    import os
    from . import monitor, ops
    if use_verts_textures or GLOBAL_POSE or not SHARED_TEXTURE:
        raise NotImplementedError("visualize_val: UV textures with one shared texture and per-frame poses are the path in scope (SURVEY.md §8)")
    for (fid, y_true, y_sil_true, _) in val_images_dataloader:
        print("epoch: %d" % epoch_id)
        for param_group in (opt_app.param_groups if opt_app is not None else ()):
            print("learning rate", param_group["lr"])
        P = params_on(params, device)
        with torch.no_grad():
            r = mirror_render(configs, monitor.merge_val_params(P, val_params, device), torch.as_tensor(fid).long(), hand_layer, mesh_subdivider,
                              device=device)
        base = configs["base_output_dir"]
        show_img_pair(r.y_pred, y_true, save_img_dir=base, step=epoch_id, silhouette=False, prefix="val_", sheet_hook=sheet_hook)
        for name, key, mode in (("uv_%04d.jpg", "texture", "image"), ("normal_%04d.jpg", "normal_map", "normal")):
            u8 = ops.sheet_u8(P[key], mode=mode, grid=(1, 1)).cpu().numpy()
            if sheet_hook is not None:
                sheet_hook(name % epoch_id, u8, {key: P[key]})
            monitor.encode_jpeg(os.path.join(base, name % epoch_id), u8)
        break


def stage_flags(epoch_id, training_stage):
    """optimize_sequence.py:507-515 -> (COARSE_OPT, APP_OPT)"""
    if epoch_id < training_stage[0]:
        return True, False
    if epoch_id < training_stage[0] + training_stage[1]:
        return True, True
    return False, True


def optimize_hand_sequence(configs, input_params, images_dataset, val_params, val_images_dataset, hand_layer,
                           VERTS_UVS=None, FACES_UVS=None, VERTS_COLOR=None, device="cuda", uv_mask=None, batch_size=18, log_fn=None,
                           seed=0, vgg=None, rank=None, world_size=None, shards=None, plateau_patience=40, plateau_threshold=1e-4, device_schedule=True,
                           evaluate=False, panels=False, turntable=False, export_mesh=False, monitor=False, device_ingest=False, texture_init=None,
                           coverage=False, pad_texture=0):
    """Fit the sequence (optimize_sequence.py:313-596).  Returns the parameter dict in the reference's checkpoint layout; evaluate=True
    then runs the post-fit evaluation `evaluate_sequence` (:595-816) on rank 0 (off by default), with its panels / turntable / export_mesh
    switches.  monitor: False (default: no new file, no new work), True, a dict of harp_amd.monitor.FitMonitor arguments or a FitMonitor —
    rank 0 then writes the reference's progress sheets while the fit runs (:490-501 every 10 epochs from the epoch's first batch; :587-589
    visualize_val every 20 epochs, which needs `val_params` and `val_images_dataset`) and monitor_log.jsonl, off the enqueueing thread.
    `images_dataset[i]` -> (fid, y_true (S,S,3), y_sil (S,S,1), y_sil_eroded (S,S,1)) like utils/data_util.ImagesDataset.
    device_ingest=True: the targets (the monitor's validation frames and the evaluation's included) come from the files of the dataset's
    image_paths / mask_paths through a thread pool of decoders and csrc/ingest.hip (ResidentTargets(ingest="device")) — the same bits,
    `images_dataset[i]` is never called; a dataset without paths raises ValueError.
    texture_init (or configs["texture_init"]): None (default: nothing in this function's path changes), "bake" or a dict of
    harp_amd.bake.bake_texture arguments — once, immediately before the first epoch whose stage has app=True, the resident frames are baked
    into UV space under the engine's current parameters (csrc/bake.hip) and the result is copied into the texture in stream order; every
    rank bakes its own shard and the float64 accumulators are summed over ranks before the finish, so all ranks write the same texture.
    Refused together with known_appearance (the texture is frozen).  coverage / pad_texture: passed on to evaluate_sequence.

    Data-parallel (the reference is single-device): launched under `torch.distributed.run` (or with rank / world_size given)
    every rank calls this function with the SAME arguments.  The dataset's items are cut into `shards` (default: world) contiguous
    shards, a rank decodes and keeps resident only its own (`ResidentTargets(frames=...)`), `batch_size` stays the GLOBAL batch of the
    reference (each shard contributes batch_size / shards frames per step), the flat gradient bucket is summed over ranks before the
    replicated dense Adam step (RCCL through `harp_allreduce_flat` inside the step's hipGraph when the process group is nccl = one
    device per rank; torch.distributed otherwise), the per-epoch shuffle comes from the shared seed WITHIN each shard
    (harp_amd.dist.epoch_batches), the epoch loss is averaged over ranks BEFORE ReduceLROnPlateau sees it (:581-582) so that every rank
    takes the same learning-rate decision, the finite check runs on that averaged loss, and only rank 0 writes checkpoints.
    `shards > world` makes one process walk several shards per step — a 1-rank job with shards = N visits the same global batches as an
    N-rank job.  plateau_patience / plateau_threshold: ReduceLROnPlateau's arguments (reference: patience 40, default threshold)."""
    from . import dist as hdist
    if configs["model_type"] != "harp":
        raise NotImplementedError("only model_type 'harp' (SURVEY.md §8: 'html' / 'nimble' are out of scope)")
    texture_init = configs.get("texture_init") if texture_init is None else texture_init
    if texture_init is not None:
        if not (texture_init == "bake" or isinstance(texture_init, dict)):
            raise ValueError(f'texture_init is None, "bake" or a dict of harp_amd.bake.bake_texture arguments, got {texture_init!r}')
        if configs["known_appearance"]:
            raise ValueError("texture_init with known_appearance: the texture is frozen (optimize_sequence.py:264-289), there is nothing to initialise")
    env_rank, env_world = hdist.dist_env()
    rank = env_rank if rank is None else int(rank)
    world = env_world if world_size is None else int(world_size)
    shards = world if shards is None else int(shards)
    n_items = len(images_dataset)
    if shards % world or n_items % shards or batch_size % shards:
        raise ValueError(f"{n_items} dataset items / global batch {batch_size} do not split evenly over {shards} shards on {world} ranks")
    k, per, b = shards // world, n_items // shards, batch_size // shards          # shards per rank, items per shard, frames per shard and step
    lo = rank * k * per                                                           # this rank's items: [lo, lo + k * per)
    S, T = configs["img_size"], input_params["pose"].shape[0]
    use_arm = bool(configs["use_arm"])
    faces0 = np.asarray((hand_layer.right_arm_faces_tensor if use_arm else hand_layer.th_faces).detach().cpu())
    topo = build_topology(faces0, 1026 if use_arm else 778)
    if uv_mask is None:
        uv_mask = load_uv_mask(configs, (512, 512))
    eng = FitEngine(hand_layer._model_np, topo, torch.as_tensor(VERTS_UVS).reshape(-1, 2), torch.as_tensor(FACES_UVS).reshape(-1, 3),
                    torch.as_tensor(uv_mask).float(), input_params, S, configs["focal_length"], b * k, device=device,
                    self_shadow=configs["self_shadow"], share_light_position=configs["share_light_position"], seed=seed,
                    use_arm=use_arm, opt_arm_pose=bool(configs.get("opt_arm_pose", False)), rank=rank, world_size=world)
    if device_ingest:                                                            # decoded once on a thread pool, converted and eroded on the device
        rt = ResidentTargets(images_dataset, frames=range(lo, lo + k * per), device=eng.dev, ingest="device")
    else:
        rt = ResidentTargets(images_dataset, frames=range(lo, lo + k * per))     # decoded once, resident in HBM (utils/data_util.py)
    if int(rt.fid.min()) < 0 or int(rt.fid.max()) >= T:
        raise ValueError(f"dataset frame ids span [{int(rt.fid.min())}, {int(rt.fid.max())}] but the parameter tables hold {T} frames")
    eng.set_targets(*rt.tensors())
    comm = None
    if world > 1:
        import torch.distributed as tdist
        if not (tdist.is_available() and tdist.is_initialized()):
            raise RuntimeError("world_size > 1 needs an initialised torch.distributed process group (torch.distributed.run)")
        if tdist.get_backend() == "nccl":                                # one device per rank: RCCL straight from the step's hipGraph
            # pre-flight + agreement over the process group: either every rank gets the communicator or none does (then the steps run
            # eagerly with torch.distributed's all-reduce); HARP_RCCL_DEBUG=1 forces that fallback (harp_amd.dist.negotiate_comm)
            comm = hdist.negotiate_comm(torch.device(device))
            if comm is not None:
                eng.set_comm(comm)
    # perceptual term (:404-405, :546-547): needs the pretrained VGG16 filters, which cannot be downloaded here — pass a ready module
    # (`vgg=`) or the path of torchvision's vgg16 state dict (configs["vgg_weights"]); without either the term is left out
    if vgg is None and configs.get("vgg_weights"):
        from .model.vgg import Vgg16Features
        vgg = Vgg16Features(layers_weights=[1, 1 / 16, 1 / 8, 1 / 4, 1], weights=configs["vgg_weights"])
    if vgg is not None:
        # configs["vgg_precision"]: 0 (default) float32 MFMA — a float32 fma chain like the reference's fp32 convolutions; 1 three-term bf16
        # split (2.5x faster, ~16 mantissa bits per product); 2 single-pass f16 (11-bit significands, float32 accumulation: the TF32 class
        # the reference's own stack runs these convolutions in).  configs["vgg_cache_bytes"]: HBM the
        # cached target activations may take (default 128 GB: 307 MB per 512x512 frame for the bounded mode, FitEngine.set_perceptual)
        eng.set_perceptual(vgg, weight=1.0, precision=int(configs.get("vgg_precision", 0)), cache_bytes=int(configs.get("vgg_cache_bytes", 128 << 30)))
    eng.keep_image = False                                           # the fused L1 consumes y_pred in the shader; nothing reads the image back
    eng.accumulate_loss = True
    eng.lean_app_stage = True                                        # the appearance-only stage steps opt_app alone (:264-310, :567-573): no geometry gradients are formed for it
    if configs["start_from"]:
        restore_checkpoint(eng, configs, input_params)
    if configs["known_appearance"]:
        # optimize_sequence.py:264-289: shape / displacement leave opt_coarse, texture / normal map leave opt_app
        eng.frozen = ("verts_disps", "shape", "texture", "normal_map")
        # ... and the key-point anchor and the mesh regularisers are not part of a test sequence's objective (:523, :531)
        eng.set_disabled_terms(("kps_anchor", "vert_disp_reg", "laplacian", "normal", "arap"))
    # ReduceLROnPlateau lives on the host; torch's own scheduler drives a dummy optimiser and the lr is mirrored to the device
    dummy = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=1e-3)
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(dummy, patience=plateau_patience, threshold=plateau_threshold)
    gen = torch.Generator().manual_seed(seed)                        # the SAME stream of draws on every rank
    # (the loss weights of :411-422 are the engine's LOSS_WEIGHTS: its kernels scale the gradients with them and its step epilogue forms sum_loss)
    own = torch.arange(k) * per                                      # first local row of each of this rank's shards
    mon = None
    if monitor is not False and monitor is not None and rank == 0:
        from .monitor import FitMonitor, due
        mon = monitor if isinstance(monitor, FitMonitor) else FitMonitor(configs["base_output_dir"], **(monitor if isinstance(monitor, dict) else {}))
    # a step may capture its graph, and no other thread may call the runtime meanwhile: the monitor's writer thread makes its calls under this lock
    step_guard = mon.hip_lock if mon is not None else contextlib.nullcontext()
    try:
        if mon is not None:
            mon.begin(configs, eng, hand_layer, VERTS_UVS, FACES_UVS, val_params, val_images_dataset, seed=seed, device_ingest=device_ingest)
        def draw_epoch():
            """the next epoch's batches (DataLoader(shuffle=True) over the DATASET's items, :398) and — its full batches as ONE device schedule
            (parameter rows = the items' own fids, :446, :464; target rows = the items): every such step is a bare graph replay that fetches
            its own row, no host tensor per step like the DataLoader's (:399); same shape every epoch, so the captured step graphs keep
            reading the same two buffers — the schedule to hand to eng.set_schedule"""
            batches = hdist.epoch_batches(per, b, gen)
            items = [(own[:, None] + order[None, :]).reshape(-1) for order in batches]  # local rows of the resident targets, shard by shard
            full = [it for it in items if it.numel() == eng.B] if device_schedule else []
            rows = torch.stack(full) if full else None
            return items, (None if rows is None else (rt.fid[rows], rows))
        items, sch = draw_epoch()
        if sch is not None:
            eng.set_schedule(sch[0], tschedule=sch[1])
        eng.loss_total.zero_()            # the engine adds every step's sum_loss (:553-559) to it on the device: no per-step host arithmetic, no sync
        baked = texture_init is None
        for epoch_id in range(configs["total_epoch"]):
            coarse, app = stage_flags(epoch_id, configs["training_stage"])
            if app and not baked:                                                      # once, in front of the first appearance epoch
                baked = True
                with step_guard:
                    bake_into_engine(eng, configs, input_params, rt, hand_layer, VERTS_UVS, FACES_UVS, uv_mask, texture_init, world)
            if mon is not None and due(epoch_id, mon.train_every):                     # :490: the forward pass of the epoch's first batch, before its step
                mon.train_sheets(epoch_id, rt.fid[items[0]], items[0])
            for item in items:
                with step_guard:
                    if item.numel() == eng.B and device_schedule:
                        eng.step(None, coarse, app)
                    else:
                        eng.step(rt.fid[item], coarse, app, tfid=item)                 # the last, partial batch (:396-399): explicit rows, a graph of its own size
            nb = len(items)
            # one sync per epoch; N > 1: the mean over ranks (image terms are means over a rank's frames, regularisers are identical),
            # the same float on every rank
            # ... and everything of the NEXT epoch that does not depend on this epoch's loss — its shuffle, its schedule (stream-ordered behind
            # the steps above) — is enqueued before that sync, so the device goes from this epoch's last step to the next one's first
            total = eng.loss_total.clone()
            eng.loss_total.zero_()
            if epoch_id + 1 < configs["total_epoch"]:
                items, sch = draw_epoch()
                if sch is not None:
                    eng.set_schedule(sch[0], tschedule=sch[1])
            # :587-589, enqueued behind this epoch's steps and in front of the sync below, which its two scalars ride on
            validated = mon is not None and due(epoch_id, mon.val_every) and mon.validate(epoch_id)
            epoch_loss = float(total.item()) / nb
            mean_loss = float(hdist.mean_over_ranks(epoch_loss, device=eng.dev)) if world > 1 else epoch_loss
            if not np.isfinite(mean_loss):
                raise FloatingPointError(f"non-finite loss at epoch {epoch_id}")      # the reference drops into pdb (:525-527); all ranks raise together
            if coarse:
                sched.step(mean_loss)                                                  # :581-582
                eng.set_lr(lr_coarse=dummy.param_groups[0]["lr"])
            if log_fn is not None:
                log_fn(epoch_id, mean_loss, eng)
            if mon is not None:
                mon.log_epoch(epoch_id, mean_loss, dummy.param_groups[0]["lr"], coarse, app, validated)
            if epoch_id % 200 == 0 and epoch_id > 0 and rank == 0:
                file_utils.save_result(export_params(eng, input_params, VERTS_UVS, FACES_UVS, uv_mask, hand_layer), configs["base_output_dir"],
                                       test=configs["known_appearance"])               # :590-591
        params = export_params(eng, input_params, VERTS_UVS, FACES_UVS, uv_mask, hand_layer)
        if rank == 0:
            file_utils.save_result(params, configs["base_output_dir"], test=configs["known_appearance"])     # :595-596
    finally:
        try:
            if mon is not None:
                mon.close()                                          # drains the writer thread; re-raises what it raised
        finally:
            if comm is not None:
                torch.cuda.synchronize(eng.dev)
                comm.destroy()                                       # drops the step graphs that captured it
    if evaluate and rank == 0:
        evaluate_sequence(configs, params, images_dataset, hand_layer, device=device, uv_mask=uv_mask, panels=panels, turntable=turntable,
                          export_mesh=export_mesh, device_ingest=device_ingest, coverage=coverage, pad_texture=pad_texture)
    return params


def bake_into_engine(eng, configs, input_params, rt, hand_layer, VERTS_UVS, FACES_UVS, uv_mask, texture_init="bake", world=1):
    """texture_init of optimize_hand_sequence: harp_amd.bake.bake_texture on the engine's current parameters and resident targets (`rt`:
    their fids), the accumulators summed over ranks, the result copied into eng.params["texture"] on the current stream.  The engine keeps
    one derived copy of the texture, the interleaved albedo + normal-map array `texnm` of the shaders: every appearance step repacks it from
    the parameter before it shades (FitEngine._param_terms), and no other step reads it, so nothing is refreshed here.  The step graphs read
    the parameter arena in place.  Returns bake_texture's dict."""
    from types import SimpleNamespace
    from . import bake as hbake
    kw = dict(texture_init) if isinstance(texture_init, dict) else {}
    fin = {k: kw.pop(k) for k in ("min_count", "fill_passes") if k in kw}
    kw.pop("device", None)
    for buf in (eng.m_buf, eng.v_buf):                               # Adam has not seen the texture yet: nothing to reset
        assert not bool(eng.arena.view(buf, "texture").any()), "texture_init: the texture's Adam moments are not zero"
    params = export_params(eng, input_params, VERTS_UVS, FACES_UVS, uv_mask, hand_layer)
    targets = SimpleNamespace(fid=rt.fid, y_true=eng.y_true, y_sil_col=eng.y_sil_col)
    acc, maps = hbake.bake_accumulate(configs, params, targets, hand_layer, device=eng.dev, **kw)
    if world > 1:
        hbake.allreduce_accumulators(acc)
    out = hbake.bake_finish(acc, maps, params, device=eng.dev, **fin)
    with torch.no_grad():
        eng.params["texture"].copy_(out["texture"].reshape(eng.params["texture"].shape))
    return out


def lpips_weights_arg(paths):
    """--lpips-weights PATH [PATH]: one combined state dict, or the (alexnet, lpips head) pair"""
    if len(paths) not in (1, 2):
        raise SystemExit("--lpips-weights takes one lpips.LPIPS state dict or two paths (torchvision alexnet, lpips v0.1 alex head)")
    return paths[0] if len(paths) == 1 else tuple(paths)


def main(argv=None):
    """optimize_sequence.py:819-838 over this package's loaders — and the data-parallel launch:

        python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 -m harp_amd.optimize_sequence --config cfg.yaml

    one rank per GPU (LOCAL_RANK), nccl (= RCCL) process group; HARP_ALL_ON_GPU0=1 puts every rank on cuda:0 over gloo (one-GPU boxes)."""
    import argparse
    import os
    import yaml
    import torch.distributed as tdist
    from .utils import hand_model_utils
    from .utils.config_utils import get_config
    from .utils.data_util import load_multiple_sequences
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", required=True, help="yaml with the keys of utils/config_utils.get_config")
    ap.add_argument("--batch-size", type=int, default=18)
    ap.add_argument("--eval", action="store_true", help="after the fit, the evaluation of optimize_sequence.py:595-816 (evaluate_sequence)")
    ap.add_argument("--panels", action="store_true", help="with --eval: one true | pred | normal | overlay JPEG per frame under rendered_after_opt/")
    ap.add_argument("--turntable", action="store_true", help="with --eval: render_360/, render_360_normal/, render_360_combine/ and render_360_light/ of frame 0")
    ap.add_argument("--export-mesh", action="store_true", help="with --eval: the Taubin-smoothed textured mesh of every frame as mesh/<fid>.obj, .mtl, .png")
    ap.add_argument("--monitor", action="store_true", help="while fitting: the progress sheets of optimize_sequence.py:490-501 every 10 epochs, "
                    "visualize_val's val_ / uv_ / normal_ sheets every 20 and monitor_log.jsonl (harp_amd.monitor.FitMonitor)")
    ap.add_argument("--device-ingest", action="store_true",
                    help="decode the frames once on a thread pool and convert / erode them on the device (csrc/ingest.hip): the same "
                         "targets, for the fit, the monitor's validation frames and --eval")
    ap.add_argument("--bake-texture", action="store_true",
                    help="before the first appearance epoch, initialise the texture by baking the frames into UV space (csrc/bake.hip; "
                         "configs['texture_init'] = 'bake')")
    ap.add_argument("--coverage", action="store_true", help="with --eval: uv_out/coverage.png, baked_texture.png, texture_std.png and the "
                    "`Texel coverage` line (which texels the video ever saw)")
    ap.add_argument("--pad-texture", type=int, default=0, metavar="K", help="with --export-mesh: dilate the exported texture K texels beyond uv_mask")
    ap.add_argument("--pose-eval", default=None, metavar="PATH",
                    help="with --eval: an .npz with any of gt_joints (T,21,3) mm, gt_joint_valid (T,21), gt_verts (T,778,3) m; adds the "
                         "Procrustes-aligned joint / vertex errors, their AUC and the F-scores (configs['pose_eval'])")
    ap.add_argument("--lpips-weights", nargs="+", default=None, metavar="PATH",
                    help="LPIPS in the evaluation: one lpips.LPIPS(net='alex') state dict, or torchvision's alexnet state dict and the lpips "
                         "v0.1 alex head (configs['lpips_weights'])")
    args = ap.parse_args(argv)
    with open(args.config) as f:
        configs = get_config(write_yaml=False, **yaml.safe_load(f))
    if args.lpips_weights:
        configs["lpips_weights"] = lpips_weights_arg(args.lpips_weights)
    if args.pose_eval:
        configs["pose_eval"] = args.pose_eval
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    shared = os.environ.get("HARP_ALL_ON_GPU0") == "1"
    device = "cuda:0" if shared else f"cuda:{local}"
    torch.cuda.set_device(device)
    if world > 1:
        import datetime
        timeout = datetime.timedelta(seconds=int(os.environ.get("HARP_DIST_TIMEOUT_S", "600")))     # a dead peer ends the job instead of hanging it
        if shared:
            tdist.init_process_group("gloo", timeout=timeout)
        else:
            tdist.init_process_group("nccl", device_id=torch.device(device), timeout=timeout)
    configs["device"] = device
    hand_layer, VERTS_UVS, FACES_UVS, VERTS_COLOR = hand_model_utils.load_hand_model(configs)
    mano_params, images_dataset, val_mano_params, val_images_dataset = load_multiple_sequences(
        configs["metro_output_dir"], configs["image_dir"], train_list=configs["train_list"], val_list=configs["val_list"],
        average_cam_sequence=configs["average_cam_sequence"], use_smooth_seq=configs["use_smooth_seq"], model_type=configs["model_type"])
    params = optimize_hand_sequence(configs, mano_params, images_dataset, val_mano_params, val_images_dataset, hand_layer, VERTS_UVS, FACES_UVS,
                                    VERTS_COLOR, device=device, batch_size=args.batch_size, evaluate=args.eval, panels=args.panels,
                                    turntable=args.turntable, export_mesh=args.export_mesh, monitor=args.monitor,
                                    device_ingest=args.device_ingest, texture_init="bake" if args.bake_texture else None,
                                    coverage=args.coverage, pad_texture=args.pad_texture)
    if world > 1:
        tdist.barrier()
        tdist.destroy_process_group()
    return params


def restore_checkpoint(eng, configs, input_params):
    """Resume from `configs["start_from"]/saved_params[_test].pkl` the way optimize_sequence.py:355-389 does — including its
    re-initialisation: the pose track is re-interpolated linearly between every 30th frame, `trans` and `rot` are replaced by their
    sequence means, parameters missing from older checkpoints get the init_params defaults; with known_appearance (and not
    pose_already_opt) pose / trans / rot / cam restart from the METRO input instead."""
    known, posed = bool(configs["known_appearance"]), bool(configs["pose_already_opt"])
    ck = file_utils.load_result(configs["start_from"], device="cpu", test=known and posed)
    ck = {k: (v.detach() if torch.is_tensor(v) else v) for k, v in ck.items()}
    if known and not posed:
        for k in ("trans", "pose", "rot", "cam"):
            ck[k] = input_params[k].detach().clone()
    T = eng.params["pose"].shape[0]
    if ck["pose"].shape[0] != T:
        raise ValueError(f"checkpoint holds {ck['pose'].shape[0]} frames, the sequence has {T}")
    pose = ck["pose"].clone()
    for i in range(T // 30 - 1):
        for j in range(30):
            pose[i * 30 + j] = ((30 - j) * ck["pose"][i * 30] + j * ck["pose"][i * 30 + 30]) / 30.0
    ck["pose"] = pose
    ck["trans"] = torch.zeros_like(ck["trans"]) + ck["trans"].mean(0)
    ck["rot"] = torch.zeros_like(ck["rot"]) + ck["rot"].mean(0)
    with torch.no_grad():
        for k in ("trans", "pose", "rot", "shape", "wrist_pose", "verts_disps", "texture", "normal_map", "light_positions", "amb_ratio", "cam"):
            if k in ck and ck[k] is not None:                     # absent keys keep the init_params defaults the engine starts with
                eng.params[k].copy_(torch.as_tensor(ck[k]).to(eng.dev).reshape(eng.params[k].shape))
    eng.compute_reference_mesh()                                  # ARAP reference = frame 0 under the restored parameters (:429-435)


def export_params(eng, input_params, VERTS_UVS, FACES_UVS, uv_mask, hand_layer):
    """the reference's parameter dict (init_params keys) from the engine's arena"""
    out = {k: eng.params[k].detach().clone() for k in ("trans", "pose", "rot", "shape", "wrist_pose", "verts_disps", "texture", "normal_map",
                                                       "light_positions", "amb_ratio", "cam")}
    out.update(init_joints=input_params["joints"], verts_rgb=torch.ones(778, 3), verts_uvs=VERTS_UVS, faces_uvs=FACES_UVS,
               uv_mask=torch.as_tensor(uv_mask), mesh_faces=getattr(hand_layer, "right_arm_faces_tensor", getattr(hand_layer, "th_faces", None)))
    return out


if __name__ == "__main__":
    main()
