"""Mirror of the fitting API of the reference's optimize_sequence.py: get_mesh_subdivider (:67-89), init_params (:181-250),
get_optimizers (:253-310) and optimize_hand_sequence (:313-816, loop body :446-582).

`optimize_hand_sequence` keeps the reference's signature and schedule (stages, batch 18, shuffle, dense Adam groups and
learning rates, ReduceLROnPlateau(patience=40) on the coarse group, checkpoint format) but runs every step through the fused
engine (harp_amd/engine.py) on HBM-resident targets.  The per-op API (`prepare_mesh`, `render_image`, losses) stays available
for callers that drive autograd themselves (`visualize_val`-style code)."""
import contextlib

import numpy as np
import torch

from .engine import FitEngine, LOSS_NAMES
from .synth import build_topology
from .utils import file_utils
from .utils.data_util import ResidentTargets
from .utils.visualize import MeshSubdivider


def get_mesh_subdivider(hand_layer, use_arm=False, device="cuda"):
    """optimize_sequence.py:67-89"""
    if use_arm:
        return MeshSubdivider(hand_layer.right_arm_faces_tensor, 1026, device)
    return MeshSubdivider(hand_layer.th_faces, 778, device)


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
        P = {k: (v.detach().to(device) if torch.is_tensor(v) else v) for k, v in params.items()}
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


def mirror_render(configs, P, fid, hand_layer, sub, device="cuda"):
    """One forward pass of frames `fid` through the reference-API mirror, as the loop body (optimize_sequence.py:452-488), visualize_val
    (:110-154) and the evaluation (:680-708) run it: get_renderers(silh_sigma=1e-7, silh_faces_per_pixel=50), prepare_mesh,
    prepare_materials, the silhouette render, and the image through get_shadow_renderers + render_image_with_RT with self_shadow, else
    render_image with the phong renderer.  P: the parameter dict on `device`.  Call under torch.no_grad().  Returns a namespace with
    y_sil_pred (B,S,S), y_pred (B,S,S,3) float32 and the intermediates (hand_verts, hand_joints (m), faces, textures, meshes, cam, light_positions,
    materials_properties, normal_renderer)."""
    from types import SimpleNamespace
    from .renderer import renderer_helper
    from .structures import Meshes
    from .utils.visualize import prepare_materials, prepare_mesh, render_image, render_image_with_RT
    S, focal = int(configs["img_size"]), configs["focal_length"]
    use_arm = bool(configs["use_arm"])
    B = fid.shape[0]
    fd = fid.to(device)
    if configs["share_light_position"]:
        light_positions = P["light_positions"][0].repeat(B, 1)
    else:
        light_positions = P["light_positions"][fd]
    phong_renderer, silhouette_renderer, normal_renderer = renderer_helper.get_renderers(
        image_size=S, light_posi=light_positions, silh_sigma=1e-7, silh_gamma=1e-1, silh_faces_per_pixel=50, device=device)
    hand_joints, hand_verts, faces, textures = prepare_mesh(P, fid, hand_layer, False, sub, False, configs, device=device, use_arm=use_arm)
    materials_properties = prepare_materials(P, B, device=device)
    meshes = Meshes(hand_verts, faces, textures)
    cam = P["cam"][fd]
    y_sil_pred = render_image(meshes, cam, B, silhouette_renderer, S, focal, silhouette=True, device=device)
    if configs["self_shadow"]:
        light_R, light_T, cam_R, cam_T = renderer_helper.process_info_for_shadow(cam, light_positions, hand_verts.mean(1), image_size=S,
                                                                                 focal_length=focal, device=device)
        shadow_renderer = renderer_helper.get_shadow_renderers(image_size=S, light_posi=light_positions, silh_sigma=1e-7, silh_gamma=1e-1,
                                                               silh_faces_per_pixel=50, amb_ratio=torch.sigmoid(P["amb_ratio"]), device=device)
        y_pred = render_image_with_RT(meshes, light_T, light_R, cam_T, cam_R, B, shadow_renderer, S, focal, silhouette=False,
                                      materials_properties=materials_properties, device=device)
    else:
        y_pred = render_image(meshes, cam, B, phong_renderer, S, focal, silhouette=False, materials_properties=materials_properties,
                              device=device)
    return SimpleNamespace(y_sil_pred=y_sil_pred, y_pred=y_pred.float(), hand_verts=hand_verts, hand_joints=hand_joints, faces=faces, textures=textures, meshes=meshes,
                           cam=cam, light_positions=light_positions, materials_properties=materials_properties, normal_renderer=normal_renderer)


EVAL_CHUNK = 64                  # optimize_sequence.py:716: image_eval runs on every 64 frames; the final stats are means of the chunk means


def evaluate_sequence(configs, params, images_dataset, hand_layer, device="cuda", batch_size=32, uv_mask=None, lpips_fn=None, panels=False,
                      turntable=False, panel_hook=None, export_mesh=False, pose_eval=None, device_ingest=False, coverage=False, pad_texture=0):
    """The post-fit evaluation of optimize_sequence.py:595-816: re-render every dataset item in order with the fitted `params` through the
    reference-API mirror (silhouette: get_renderers(silh_sigma=1e-7, silh_faces_per_pixel=50)[1]; image: render_image_with_RT through
    get_shadow_renderers with self_shadow, else render_image with the phong renderer), `batch_size` frames per render call; per-frame
    Silhouette IoU, L1 and MS-SSIM from ops.image_metrics (csrc/metrics.hip); the reference's averaging — the mean over 64-frame chunks
    (the last partial chunk included) of each chunk's mean; with configs["eval_mesh"] the Procrustes-aligned vertex error against
    `<gt_mesh_dir>/<500 + fid + 1>_manov.xyz` (:760-774, also written to eval_vert_mm[_test].txt).  Writes eval_results[_test].txt
    (" %s: %.5f" lines, :808-816) and uv_out/texture.png, uv_out/normal_map.png (:627-654) under configs["base_output_dir"] and returns
    the stats dict.  LPIPS (harp_amd.lpips, csrc/lpips.hip) is added when `lpips_fn` is given or configs["lpips_weights"] names its weights
    (a combined lpips.LPIPS state-dict path, or a (torchvision alexnet, lpips v0.1 head) path pair): per frame on the same y_true / y_pred,
    [0, 1] images without `normalize` as the reference passes them, averaged like the others and written in the reference's key order (IoU,
    L1, LPIPS, MS_SSIM); without either the output has no LPIPS line (the weights cannot be shipped).  Left out: MS_SSIM with a warning when
    the image side is <= 160 px (the reference would fail pytorch_msssim's assertion there).
    What the reference writes for the eye is off by default and leaves metrics and files as they are when off.  panels=True: per batch one
    more prepare_mesh(vis_normal=True) + normal render (:710-714), one ops.panels_u8 and one `true | pred | normal | overlay` JPEG per frame,
    rendered_after_opt[_test]/<fid %04d>.jpg (:742-757); panel_hook(fid, strip), if given, sees every (S, 4S, 3) uint8 strip before it is
    encoded.  turntable=True: for the dataset item whose fid is 0 (:716-727) render_360 with the phong and the normal renderer,
    concat_image_in_dir into render_360_combine and render_360_light, each with its out.gif.  export_mesh=True (the reference's constant
    EXPORT_MESH, :776-791): per batch one ops.taubin_smoothing(meshes) (csrc/smooth.hip) and one device -> host copy, then per frame
    mesh/<fid %04d>.obj, .mtl and .png through harp_amd.io.save_obj with the reference's arguments — smoothed vertices, the faces of the
    unsmoothed mesh, the textures' verts_uvs / faces_uvs and maps_padded()[0].clamp(0, 1), whose PNG is encoded once (the texture is shared).
    pose_eval (or configs["pose_eval"]): None, the path of an .npz or a dict with any of gt_joints (T,21,3) mm, gt_joint_valid (T,21) and
    gt_verts (T,778,3) m, rows indexed by fid.  Given, the geometric accuracy runs on the device (csrc/pose_eval.hip), per batch one
    ops.procrustes_align of the first 21 joints (mm, both sets root-aligned, only the valid joints), one of the vertices (gathered by
    right_mano_idx on the arm, else the first 778; with configs["eval_mesh"] and no gt_verts they still come from load_gt_vert) and one
    ops.point_set_fscore of the aligned vertices; after the lines above, whichever the ground truth allows of `Procrustes-aligned joint
    error (mm)`, `Joint AUC 0-50 mm` (100 thresholds), `Procrustes-aligned vertex error (mm)`, `Vertex AUC 0-50 mm`, `F@5mm`, `F@15mm`,
    and eval_joint_mm[_test].txt / eval_vert_mm[_test].txt with the per-frame means.  Frames with fewer than 3 valid joints are left out
    of the joint lines.  With None everything is as before: the per-frame host loop of :760-774 included.
    device_ingest=True: per batch the ground truth comes from utils.data_util.decode_u8 and ops.targets_from_u8(eroded=False) instead of
    `images_dataset[i]` — the same bits, each file decoded once and no erosion computed; needs a dataset with paths (ValueError otherwise).
    coverage=True: one harp_amd.bake.bake_texture pass over the dataset with the fitted parameters and delight=True (csrc/bake.hip) — writes
    uv_out/coverage.png (8-bit, min(count, 255): in how many frames a texel was observed), uv_out/baked_texture.png (the projective albedo,
    filled inside the charts) and uv_out/texture_std.png (the weighted standard deviation of the observed colours), and adds the line
    ` Texel coverage: %.5f` (the share of uv_mask & covered texels seen at least once) as the last one.  pad_texture=k (export_mesh): the
    exported PNG is dilated by k 3 x 3 passes from uv_mask > 0.5 into the rest (harp_amd.bake.pad_texture), which removes the dark band a
    viewer's bilinear lookup pulls across the chart borders; 0 (default): today's bytes.  uv_out/texture.png stays the reference's."""
    import os
    import warnings
    import torch.nn.functional as F
    from PIL import Image
    from . import ops
    from .io import encode_png, save_obj
    from .renderer import renderer_helper
    from .structures import Meshes
    from .utils.data_util import _ingest_paths, decode_u8
    from .utils.eval_util import EvalUtil, align_w_scale, load_gt_vert, sil_iou
    from .utils.visualize import concat_image_in_dir, prepare_mesh, render_360, render_360_light, render_image
    S, focal = int(configs["img_size"]), configs["focal_length"]
    base = configs["base_output_dir"]
    test_name = "_test" if configs["known_appearance"] else ""
    use_arm = bool(configs["use_arm"])
    P = {k: (v.detach().to(device) if torch.is_tensor(v) else v) for k, v in params.items()}
    # ---- texture and normal map (:627-654)
    uv_out_dir = os.path.join(base, "uv_out")
    os.makedirs(uv_out_dir, exist_ok=True)
    uvm = params.get("uv_mask") if uv_mask is None else uv_mask
    tex = P["texture"].cpu().numpy()[0]
    uvm = np.ones(tex.shape[:2]) if uvm is None else np.asarray(torch.as_tensor(uvm).detach().cpu(), dtype=np.float64)
    Image.fromarray(np.uint8(tex.clip(0, 1) * np.expand_dims(uvm, 2) * 255)).save(os.path.join(uv_out_dir, "texture.png"))
    if "normal_map" in P:
        nm = F.normalize(P["normal_map"], dim=-1).cpu().numpy()
        nm = (nm / 2.0 + 0.5) * np.expand_dims(uvm, 2)
        Image.fromarray(np.uint8(nm[0].clip(0, 1) * 255)).save(os.path.join(uv_out_dir, "normal_map.png"))
    # ---- renders and per-frame metrics
    sub = get_mesh_subdivider(hand_layer, use_arm=use_arm, device=device)
    with_ms = S > ops.MS_SSIM_MIN_SIDE
    if not with_ms:
        warnings.warn(f"MS_SSIM left out of the evaluation: {S} px images (pytorch_msssim needs a side > {ops.MS_SSIM_MIN_SIDE})")
    if lpips_fn is None and configs.get("lpips_weights"):
        from .lpips import LPIPS
        lw = configs["lpips_weights"]
        lpips_fn = LPIPS(weights=tuple(lw) if isinstance(lw, (list, tuple)) else lw).to(device)
    with_lpips = lpips_fn is not None and S >= ops.LPIPS_MIN_SIDE
    if lpips_fn is not None and not with_lpips:
        warnings.warn(f"LPIPS left out of the evaluation: {S} px images (AlexNet needs a side >= {ops.LPIPS_MIN_SIDE})")
    iou, l1, ms, lp, vert_err = [], [], [], [], []
    pe = pose_eval if pose_eval is not None else configs.get("pose_eval")
    if isinstance(pe, (str, os.PathLike)):
        with np.load(pe) as z:
            pe = {k: z[k] for k in z.files}
    if pe is not None:
        pe = {k: torch.as_tensor(np.asarray(v)) for k, v in pe.items() if k in ("gt_joints", "gt_joint_valid", "gt_verts")}
        with_joints = "gt_joints" in pe
        with_verts = "gt_verts" in pe or bool(configs["eval_mesh"])
        joint_err, f_scores = [], []
        joint_pck, vert_pck = EvalUtil(21), EvalUtil(778)
        vert_idx = (torch.as_tensor(np.asarray(hand_layer.right_mano_idx)) if use_arm else torch.arange(778)).to(device=device, dtype=torch.int32)
        f_thr = torch.tensor([0.005, 0.015], dtype=torch.float32, device=device)        # metres
    panel_dir = os.path.join(base, "rendered_after_opt" + test_name)
    if panels:
        os.makedirs(panel_dir, exist_ok=True)                      # :660
    mesh_dir, png = os.path.join(base, "mesh"), None
    if export_mesh:
        os.makedirs(mesh_dir, exist_ok=True)                       # :783
    n = len(images_dataset)
    if device_ingest:
        ingest_d = _ingest_paths(images_dataset)[2]                # ValueError for a dataset without paths, before anything is rendered
    with torch.no_grad():
        for lo in range(0, n, batch_size):
            if device_ingest:
                fid = torch.arange(lo, min(n, lo + batch_size), dtype=torch.long)       # ImagesDataset: the item's index is its fid
                rgb_u8, mask_u8 = (torch.from_numpy(a).to(device) for a in decode_u8(images_dataset, fid.tolist()))
                y_true, y_sil_true, _ = ops.targets_from_u8(rgb_u8, mask_u8, d=ingest_d, eroded=False)
            else:
                items = [images_dataset[i] for i in range(lo, min(n, lo + batch_size))]
                fid = torch.as_tensor([int(it[0]) for it in items], dtype=torch.long)
                y_true = torch.stack([torch.as_tensor(it[1]) for it in items]).to(device=device, dtype=torch.float32)
                y_sil_true = torch.stack([torch.as_tensor(it[2]) for it in items]).reshape(len(items), S, S).to(device=device, dtype=torch.float32)
            B = fid.shape[0]
            r = mirror_render(configs, P, fid, hand_layer, sub, device=device)
            hand_verts, faces, textures, meshes, cam = r.hand_verts, r.faces, r.textures, r.meshes, r.cam
            light_positions, materials_properties, normal_renderer = r.light_positions, r.materials_properties, r.normal_renderer
            y_sil_pred, y_pred = r.y_sil_pred, r.y_pred
            if panels:                                # :710-714, :742-757
                _, verts_n, faces_n, textures_n = prepare_mesh(P, fid, hand_layer, False, sub, False, configs, device=device, vis_normal=True,
                                                               use_arm=use_arm)
                y_pred_normal = render_image(Meshes(verts_n, faces_n, textures_n), cam, B, normal_renderer, S, focal, silhouette=False,
                                             materials_properties=materials_properties, device=device)
                strips = ops.panels_u8([y_true, y_pred, y_pred_normal], y_sil_true, y_sil_pred).cpu().numpy()
                for b in range(B):
                    if panel_hook is not None:
                        panel_hook(int(fid[b]), strips[b])
                    Image.fromarray(strips[b]).save(os.path.join(panel_dir, "%04d.jpg" % int(fid[b])))
            if turntable and bool((fid == 0).any()):   # :716-727: one frame turned through 360 degrees and lit from 40 positions
                i0 = int((fid == 0).nonzero()[0])
                f0 = fid[i0:i0 + 1]
                phong0, _, normal0 = renderer_helper.get_renderers(image_size=S, light_posi=light_positions[i0:i0 + 1], silh_sigma=1e-7,
                                                                   silh_gamma=1e-1, silh_faces_per_pixel=50, device=device)
                kw360 = dict(configs=configs, use_arm=use_arm, verts_textures=False, mesh_subdivider=sub, global_pose=False, save_img_dir=base,
                             device=device)
                render_360(P, f0, phong0, S, focal, hand_layer, **kw360)
                render_360(P, f0, normal0, S, focal, hand_layer, render_normal=True, **kw360)
                concat_image_in_dir(os.path.join(base, "render_360"), os.path.join(base, "render_360_normal"), os.path.join(base, "render_360_combine"))
                render_360_light(P, f0, hand_verts[i0:i0 + 1], faces, textures, S, focal, save_img_dir=base, device=device)
            if with_ms:
                m = ops.image_metrics(y_true, y_pred, y_sil_true, y_sil_pred)
                iou.append(m["iou"].cpu())
                l1.append(m["l1_sum"].double().cpu())
                ms.append(m["ms_ssim"].double().cpu())
            else:                                     # no MS-SSIM at this size, so no metrics kernel: sil_iou / l1_diff per frame
                iou.append(torch.stack([torch.as_tensor(sil_iou(y_sil_true[b:b + 1], y_sil_pred[b:b + 1])) for b in range(B)]).cpu())
                l1.append((y_true - y_pred).abs().double().sum((1, 2, 3)).cpu())
            if with_lpips:                            # :51-53 of utils/eval_util.py, per frame
                lp.append(lpips_fn(y_true.permute(0, 3, 1, 2), y_pred.permute(0, 3, 1, 2)).reshape(B).double().cpu())
            if pe is not None:                        # the device path of :760-774 and of utils/eval_util.py:166-209
                if with_joints:
                    gt_j = pe["gt_joints"][fid].to(device=device, dtype=torch.float32)
                    gt_j = gt_j - gt_j[:, :1]
                    pred_j = r.hand_joints[:, :21].float() * 1000.0
                    pred_j = pred_j - pred_j[:, :1]
                    vis = (pe["gt_joint_valid"][fid] == 1).to(device) if "gt_joint_valid" in pe else torch.ones(B, 21, dtype=torch.bool, device=device)
                    al_j, err_j, nv = ops.procrustes_align(gt_j, pred_j, valid=vis.float())
                    ok = nv >= 3
                    joint_err.append((torch.nan_to_num(err_j.double()).sum(1) / nv.clamp(min=1))[ok].cpu())
                    joint_pck.feed_batch(gt_j, vis & ok[:, None], al_j)
                if with_verts:
                    if "gt_verts" in pe:
                        gt_v = pe["gt_verts"][fid].to(device=device, dtype=torch.float32)
                    else:
                        gt_v = torch.as_tensor(np.stack([load_gt_vert(fid[b:b + 1], configs["gt_mesh_dir"], dataset="synthetic", start_from_one=True,
                                                                      idx_offset=500) for b in range(B)]), dtype=torch.float32).to(device)
                    al_v, err_v, _ = ops.procrustes_align(gt_v, hand_verts, pred_idx=vert_idx)
                    vert_err.extend((err_v.double().mean(1) * 1000.0).cpu().tolist())
                    vert_pck.feed_batch(gt_v * 1000.0, torch.ones(B, 778, device=device), al_v * 1000.0)
                    f_scores.append(ops.point_set_fscore(gt_v, al_v, f_thr)[0][:, :, 2].double().cpu())
            elif configs["eval_mesh"]:               # :760-774
                for b in range(B):
                    gt = load_gt_vert(fid[b:b + 1], configs["gt_mesh_dir"], dataset="synthetic", start_from_one=True, idx_offset=500)
                    pred = hand_verts[b, hand_layer.right_mano_idx] if use_arm else hand_verts[b, :778]
                    err = gt - align_w_scale(gt, pred.detach().cpu().numpy())
                    vert_err.append(float(np.linalg.norm(err, axis=1).mean()) * 1000.0)
            if export_mesh:                           # :776-791
                smoothed = ops.taubin_smoothing(meshes).verts_padded().cpu()
                faces_cpu = meshes.faces_padded()[0].cpu()
                verts_uvs = meshes.textures.verts_uvs_padded()[0].detach().cpu()
                faces_uvs = meshes.textures.faces_uvs_padded()[0].detach().cpu()
                if png is None:                       # prepare_mesh repeats ONE texture over every frame of every batch: encoded once
                    from .bake import pad_texture as pad_map
                    png = encode_png(pad_map(meshes.textures.maps_padded()[0].detach(), uvm, pad_texture).cpu().clamp(0, 1))
                for b in range(B):
                    save_obj(os.path.join(mesh_dir, "%04d.obj" % int(fid[b])), verts=smoothed[b], faces=faces_cpu, verts_uvs=verts_uvs,
                             faces_uvs=faces_uvs, texture_png=png)
    # ---- the reference's averaging: image_eval per 64-frame chunk (:713-731), then np.mean over the chunks (:733-738)
    iou, l1 = torch.cat(iou).double(), torch.cat(l1)
    chunks = [slice(c, min(n, c + EVAL_CHUNK)) for c in range(0, n, EVAL_CHUNK)]
    per_pixel = float(S * S * 3)
    stats = {"Silhouette IoU": float(np.mean([iou[c].mean().item() for c in chunks])),
             "L1": float(np.mean([l1[c].sum().item() / ((c.stop - c.start) * per_pixel) for c in chunks]))}
    if with_lpips:
        lp = torch.cat(lp)
        stats["LPIPS"] = float(np.mean([lp[c].mean().item() for c in chunks]))
    if with_ms:
        ms = torch.cat(ms)
        stats["MS_SSIM"] = float(np.mean([ms[c].mean().item() for c in chunks]))
    if pe is not None and with_joints:
        joint_err = torch.cat(joint_err).tolist()
        if joint_err:
            stats["Procrustes-aligned joint error (mm)"] = float(np.mean(joint_err))
            stats["Joint AUC 0-50 mm"] = float(joint_pck.get_measures(0.0, 50.0, 100)[2])
            np.savetxt(os.path.join(base, "eval_joint_mm" + test_name + ".txt"), joint_err)
    if vert_err:
        stats["Procrustes-aligned vertex error (mm)"] = float(np.mean(vert_err))
        np.savetxt(os.path.join(base, "eval_vert_mm" + test_name + ".txt"), vert_err)
        if pe is not None:
            f = torch.cat(f_scores).mean(0)
            stats["Vertex AUC 0-50 mm"] = float(vert_pck.get_measures(0.0, 50.0, 100)[2])
            stats["F@5mm"], stats["F@15mm"] = float(f[0]), float(f[1])
    if coverage:                                      # which texels did the video ever see (csrc/bake.hip)
        from .bake import bake_texture
        baked = bake_texture(configs, dict(P, uv_mask=torch.as_tensor(uvm)), images_dataset, hand_layer, delight=True, device=device,
                             device_ingest=device_ingest)
        u8 = lambda t: t.detach().float().clamp(0, 1).mul(255).to(torch.uint8).cpu().numpy()      # noqa: E731
        Image.fromarray(baked["count"].clamp(max=255).to(torch.uint8).cpu().numpy()).save(os.path.join(uv_out_dir, "coverage.png"))
        Image.fromarray(u8(baked["texture"][0])).save(os.path.join(uv_out_dir, "baked_texture.png"))
        Image.fromarray(u8(baked["variance"].sqrt())).save(os.path.join(uv_out_dir, "texture_std.png"))
        stats["Texel coverage"] = baked["coverage"]
    print("  -- Evaluation --")
    for k, v in stats.items():
        print(" %s: %.5f" % (k, v))
    with open(os.path.join(base, "eval_results" + test_name + ".txt"), "w") as f_out:
        for k, v in stats.items():
            f_out.write(" %s: %.5f\n" % (k, v))
    return stats


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
