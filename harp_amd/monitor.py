"""In-fit monitoring: what the reference's loop shows of a running fit (optimize_sequence.py:490-501 show_img_pair every 10 epochs,
:587-589 visualize_val every 20), kept off the path that enqueues the steps.

A monitor event renders a handful of frames through the reference-API mirror on the CURRENT stream (stream-ordered with the steps: a
side-stream render would race Adam's parameter update), turns each batch of float images into ONE uint8 contact sheet on the device
(ops.sheet_u8, csrc/sheet.hip) and hands the sheet to a writer thread: device -> pinned host copy on a side stream behind an event, a
second event after it, JPEG encoding and the file write on the thread.  Only uint8 sheets leave the device, and the enqueueing thread
waits for the encoder only when all `slots` pinned buffers are in use (counted in `waits` / `wait_s`).

The step graphs are captured in the capture mode that forbids event calls from ANY thread while a capture is open (a call from the writer
thread then fails and invalidates the capture).  So the writer thread touches the runtime only under `hip_lock` — it polls the copy's
event and reads the timers there, and holds the lock for those calls alone, never while it waits or encodes — and whoever captures a
graph while a monitor is open holds the same lock (optimize_hand_sequence takes it around every step).

The sheets are not matplotlib's figures: the cells lie edge to edge, box-averaged by the smallest integer factor that brings three cells
under `max_side` pixels (the reference's figure is 1000 px wide with margins)."""
import json
import os
import queue
import threading
import time
from types import SimpleNamespace

import torch

from .evaluate import mirror_render
from .utils.visualize import get_mesh_subdivider

SHEET_GRID = (3, 3)                    # show_img_pair: fig.add_subplot(3, 3, ...) (:41-43)
FIT_KEYS = ("trans", "pose", "rot", "shape", "wrist_pose", "verts_disps", "texture", "normal_map", "light_positions", "amb_ratio", "cam")


def box_factor(S, max_side=1024, cells=3):
    """the smallest integer d >= 1 with cells * ceil(S / d) <= max_side"""
    d = 1
    while cells * -(-int(S) // d) > max_side:
        d += 1
    return d


def due(epoch, every):
    """`epoch % every == 0` (:490, :587); every <= 0 turns the event off"""
    return every > 0 and epoch % every == 0


def encode_jpeg(path, u8, quality=90):
    from PIL import Image
    Image.fromarray(u8).save(path, quality=quality)


def merge_val_params(params, val_params, device):
    """the parameter dict visualize_val renders with (:119-135): shape, pose, wrist_pose, verts_disps, texture, normal_map (and the light,
    :110-113) of the fit under the validation sequence's own cam, trans and rot"""
    out = dict(params)
    for k in ("cam", "trans", "rot"):
        out[k] = torch.as_tensor(val_params[k]).detach().to(device=device, dtype=torch.float32)
    return out


def val_metrics(y_true, y_sil_true, y_sil_col, y_pred, y_sil_pred):
    """(2,) device tensor: the masked photometric L1 of :543 and the silhouette IoU of utils/eval_util.sil_iou, without a host round trip"""
    m = y_sil_col.unsqueeze(-1)
    l1 = (y_true * m - y_pred * m).abs().mean()
    r, p = y_sil_true >= 0.5, y_sil_pred.reshape(y_sil_true.shape) >= 0.5
    iou = torch.mean(torch.logical_and(r, p).sum([1, 2]) / torch.logical_or(r, p).sum([1, 2]))
    return torch.stack([l1, iou]).float()


class FitMonitor:
    """FitMonitor(base_output_dir, train_every=10, val_every=20, max_side=1024, slots=8, quality=90, sheet_hook=None, encode_fn=None).
    Files are `base_output_dir + prefix + name`, concatenated as the reference does (:58-60).  sheet_hook(name, u8, sources), if given,
    is called from the writer thread with every (H,W,3) uint8 sheet and a dict of the float tensors it was made from; encode_fn(path, u8)
    replaces the JPEG encoder.  `optimize_hand_sequence(monitor=...)` drives begin / train_sheets / validate / log_epoch / close; submit()
    is the asynchronous half on its own."""

    def __init__(self, base_output_dir, train_every=10, val_every=20, max_side=1024, slots=8, quality=90, sheet_hook=None, encode_fn=None,
                 prefix=""):
        if slots < 1:
            raise ValueError("FitMonitor needs at least one pinned slot")
        self.base, self.prefix = base_output_dir, prefix
        self.train_every, self.val_every, self.max_side, self.quality = int(train_every), int(val_every), int(max_side), quality
        self.sheet_hook, self.encode_fn = sheet_hook, encode_fn
        self._free, self._work = queue.Queue(), queue.Queue()
        for i in range(slots):
            self._free.put(i)
        self._pinned = [None] * slots
        self._thread = self._copy_stream = self._error = self._log = None
        self._lock = threading.Lock()
        self.hip_lock = threading.Lock()             # held by the writer thread around its runtime calls, and by the fit around its steps
        self.submitted = self.finished = self.waits = 0
        self.wait_s = 0.0
        self.timings = []                            # one record per written sheet: device and encoder times in ms
        self.val = None

    # ---- the asynchronous half --------------------------------------------------------------------------------------------------
    @property
    def pending(self):
        with self._lock:
            return self.submitted - self.finished

    def submit(self, name, sheet, sources=None, marks=None):
        """Queue the (H,W,3) uint8 device tensor `sheet` to be written as base + name.  marks: timed events already recorded around the
        work that made it ({"render": (e0, e1), "sheet": (e0, e1)})."""
        dev = sheet.device
        if self._thread is None:
            d = os.path.dirname(self.base)
            if d:
                os.makedirs(d, exist_ok=True)
            self._copy_stream = torch.cuda.Stream(device=dev)
            self._thread = threading.Thread(target=self._run, name="harp-fit-monitor", daemon=True)
            self._thread.start()
        try:
            slot = self._free.get_nowait()
        except queue.Empty:                          # back-pressure: every pinned buffer is waiting for the encoder
            t0 = time.perf_counter()
            slot = self._free.get()
            self.waits += 1
            self.wait_s += time.perf_counter() - t0
        n = sheet.numel()
        buf = self._pinned[slot]
        if buf is None or buf.numel() < n:
            buf = self._pinned[slot] = torch.empty(n, dtype=torch.uint8, pin_memory=True)
        ready = torch.cuda.Event()
        ready.record(torch.cuda.current_stream(dev))
        cs = self._copy_stream
        cs.wait_event(ready)
        c0, c1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(cs):
            c0.record(cs)
            buf[:n].copy_(sheet.reshape(-1), non_blocking=True)
            c1.record(cs)
        sheet.record_stream(cs)
        marks = dict(marks or {}, copy=(c0, c1))
        with self._lock:
            self.submitted += 1
        self._work.put(SimpleNamespace(name=name, slot=slot, buf=buf, n=n, shape=tuple(sheet.shape), done=c1, marks=marks,
                                       sources=sources if self.sheet_hook is not None else None))

    def _run(self):
        while True:
            job = self._work.get()
            if job is None:
                return
            try:
                while True:                          # the copy's event, polled: never a runtime call while a graph is being captured
                    with self.hip_lock:
                        if job.done.query():
                            break
                    time.sleep(2e-4)
                with self.hip_lock:
                    times = {k + "_ms": e0.elapsed_time(e1) for k, (e0, e1) in job.marks.items()}
                u8 = job.buf[:job.n].numpy().reshape(job.shape)
                if self.sheet_hook is not None:
                    self.sheet_hook(job.name, u8.copy(), job.sources)
                t0 = time.perf_counter()
                if self.encode_fn is not None:
                    self.encode_fn(self.base + job.name, u8)
                else:
                    encode_jpeg(self.base + job.name, u8, self.quality)
                self.timings.append(dict(times, name=job.name, encode_ms=(time.perf_counter() - t0) * 1e3))
            except BaseException as e:               # kept for close(); the queue keeps draining so that no slot is lost
                if self._error is None:
                    self._error = e
            finally:
                with self.hip_lock:                  # the events (and the hook's tensors) are destroyed here, not wherever `job` is dropped
                    job.marks = job.done = job.sources = None
                self._free.put(job.slot)
                with self._lock:
                    self.finished += 1

    def close(self):
        """drain the queue, join the writer thread and re-raise what it raised"""
        if self._thread is not None:
            self._work.put(None)
            self._thread.join()
            self._thread = None
        if self._log is not None:
            self._log.close()
            self._log = None
        err, self._error = self._error, None
        if err is not None:
            raise err

    def _sheet(self, name, a, b=None, mask=None, mode="image", grid=SHEET_GRID, d=1, sources=None, render=None):
        from . import ops
        s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s0.record()
        sheet = ops.sheet_u8(a, b, mask, mode=mode, grid=grid, d=d)
        s1.record()
        if self.sheet_hook is not None:              # the atlas is a live view that Adam keeps updating: the hook gets what the sheet saw
            sources = {k: v.detach().clone() for k, v in sources.items()}
        marks = {"sheet": (s0, s1)}
        if render is not None:
            marks["render"] = render
        self.submit(self.prefix + name, sheet, sources, marks)

    # ---- the fit's side ---------------------------------------------------------------------------------------------------------
    def begin(self, configs, eng, hand_layer, verts_uvs, faces_uvs, val_params=None, val_images_dataset=None, seed=0, device_ingest=False):
        """bind to a fit: the engine's parameter views and resident targets; up to 9 validation items drawn ONCE from a generator of
        their own (seed + 1: the training shuffle's generator is not consumed) and kept resident"""
        from .utils.data_util import ResidentTargets
        self.cfg, self.eng, self.layer, self.dev = configs, eng, hand_layer, eng.dev
        self.d = box_factor(configs["img_size"], self.max_side, SHEET_GRID[1])
        if self.d > 8:
            raise ValueError(f"max_side = {self.max_side} asks for a box factor of {self.d} at {configs['img_size']} px (at most 8)")
        self.sub = get_mesh_subdivider(hand_layer, use_arm=bool(configs["use_arm"]), device=self.dev)
        dv = lambda t: t.to(self.dev) if torch.is_tensor(t) else t
        self.P = {k: eng.params[k] for k in FIT_KEYS}
        self.P.update(verts_uvs=dv(verts_uvs), faces_uvs=dv(faces_uvs),
                      mesh_faces=getattr(hand_layer, "right_arm_faces_tensor", getattr(hand_layer, "th_faces", None)))
        self.val = None
        if val_params is not None and val_images_dataset is not None and len(val_images_dataset) > 0:
            g = torch.Generator().manual_seed(seed + 1)
            idx = torch.randperm(len(val_images_dataset), generator=g)[:SHEET_GRID[0] * SHEET_GRID[1]].tolist()
            rt = ResidentTargets(val_images_dataset, frames=idx, device=self.dev, ingest="device" if device_ingest else "host")
            T, Tv = eng.params["pose"].shape[0], min(torch.as_tensor(val_params[k]).shape[0] for k in ("cam", "trans", "rot"))
            if int(rt.fid.min()) < 0 or int(rt.fid.max()) >= min(T, Tv):
                raise ValueError(f"validation frame ids span [{int(rt.fid.min())}, {int(rt.fid.max())}] but the fit's pose table holds {T} frames "
                                 f"and the validation tables {Tv} (visualize_val indexes both with them, optimize_sequence.py:137-140)")
            self.val = SimpleNamespace(fid=rt.fid.long(), rt=rt, P=merge_val_params(self.P, val_params, self.dev),
                                       host=torch.empty(2, dtype=torch.float32, pin_memory=True))
        d = os.path.dirname(self.base)
        if d:
            os.makedirs(d, exist_ok=True)
        self._log = open(self.base + self.prefix + "monitor_log.jsonl", "w")

    def _render(self, P, fid):
        r0, r1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.no_grad():
            r0.record()
            r = mirror_render(self.cfg, P, fid, self.layer, self.sub, device=self.dev)
            r1.record()
        return r, (r0, r1)

    def train_sheets(self, epoch, fid, rows):
        """%04d.jpg, sil_%04d.jpg and loss_%04d.jpg (:490-501) of the first min(9, B) items of the epoch's first batch: parameter rows `fid`,
        rows `rows` of the engine's resident targets, the parameters as they are now (before the epoch's first step)"""
        n = SHEET_GRID[0] * SHEET_GRID[1]
        fid, rows = torch.as_tensor(fid)[:n].long(), torch.as_tensor(rows)[:n].long().to(self.dev)
        r, marks = self._render(self.P, fid)
        y_true, y_sil, y_col = self.eng.y_true[rows], self.eng.y_sil[rows], self.eng.y_sil_col[rows]
        self._sheet("%04d.jpg" % epoch, r.y_pred, d=self.d, sources={"y_pred": r.y_pred}, render=marks)
        self._sheet("sil_%04d.jpg" % epoch, y_sil, r.y_sil_pred, mode="overlay", d=self.d, sources={"y_sil_true": y_sil, "y_sil_pred": r.y_sil_pred})
        self._sheet("loss_%04d.jpg" % epoch, y_true, r.y_pred, y_col, mode="absdiff", d=self.d,
                    sources={"y_true": y_true, "y_pred": r.y_pred, "y_sil_true_col": y_col})

    def validate(self, epoch):
        """val_%04d.jpg, uv_%04d.jpg, normal_%04d.jpg (:97-171) under the parameters as they are now; the two metrics start their way to a
        pinned host buffer on the current stream — log_epoch reads them after the loop's own per-epoch sync.  False without a validation set."""
        if self.val is None:
            return False
        v = self.val
        r, marks = self._render(v.P, v.fid)
        with torch.no_grad():
            v.host.copy_(val_metrics(v.rt.y_true, v.rt.y_sil, v.rt.y_sil_col, r.y_pred, r.y_sil_pred), non_blocking=True)
        self._sheet("val_%04d.jpg" % epoch, r.y_pred, d=self.d, sources={"y_pred": r.y_pred}, render=marks)
        self._sheet("uv_%04d.jpg" % epoch, self.P["texture"], grid=(1, 1), sources={"texture": self.P["texture"]})
        self._sheet("normal_%04d.jpg" % epoch, self.P["normal_map"], mode="normal", grid=(1, 1), sources={"normal_map": self.P["normal_map"]})
        return True

    def log_epoch(self, epoch, total_loss_epoch, lr_coarse, coarse, app, validated=False):
        """one line of monitor_log.jsonl (the reference's tf_writer scalars, :585).  validated: validate() ran for this epoch and the
        stream it ran on has been synchronised since"""
        rec = {"epoch": int(epoch), "total_loss_epoch": float(total_loss_epoch), "lr_coarse": float(lr_coarse), "coarse": bool(coarse), "app": bool(app)}
        if validated:
            rec["val_l1"], rec["val_iou"] = (float(x) for x in self.val.host.tolist())
        self._log.write(json.dumps(rec) + "\n")
        self._log.flush()
