"""-m gpu: the hand-offs between host and device of the players, the device ingest and the in-fit monitor, with the DEVICE made late
(tests/_delay.py: busy_wait, late_calls, wait_spy).

Each of these paths lets the host run ahead of the device through pinned memory and events: the players rewrite one pinned index table
per call (A), `_play` hands pinned frame buffers to the encoders (B), the device ingest decodes into two pinned staging buffers (C), the
monitor copies a sheet on a side stream into a pinned slot that a writer thread reads (D).  On an idle device every copy has long finished
when the host comes round to its buffer, so any of the guarding waits could be deleted and every other test would stay green.  Here a
busy wait of D milliseconds is put in front of the device work, the calls are made back to back and read by in-stream clones with one
synchronise at the end, and the results must equal, bit for bit, those of the same calls made one at a time on an idle device.

D is a stimulus, not a tolerance: the larger of 20 ms and 10 x the host wall time of one undelayed call of the path, at most 200 ms.  A
run counts only if the spy on torch.cuda.Event.synchronize (for D: Event.query on the writer thread) saw a wait whose event was not yet
complete — otherwise the test fails as INCONCLUSIVE.  Four positive controls bypass a host-side wait from the test (nothing in harp_amd/ is
edited) and must SEE a difference; every value that reaches the device in a control is valid for that call's buffers (tables of one length
over one motion, frames of one size, the test's own allocated blocks).  Measured figures: docs/NOTEBOOK.md, "Host/device hand-offs under
a late device"."""
import os
import threading
import time

import numpy as np
import pytest
import torch

from tests import _ingest_ref as R
from tests._delay import _EVENT_BASE, busy_wait, incomplete, late_calls, wait_spy
from tests.test_gpu_evaluate import _setup

pytestmark = pytest.mark.gpu
DEV = "cuda"
S, T, BATCH = 64, 7, 2
ROWS = ([0, 1, 2], [3, 4, 5], [6, 2, 0])                 # equal lengths: one n_pad, one graph key; every position differs
TO_ROWS = ([1, 2, 3], [4, 5, 6], [5, 0, 1])
SIDE_ROWS = ([0, 1, 2], [3, 0, 1], [2, 3, 0])            # rows of the 4-row background / scene-depth tensors
WRITER = "harp-fit-monitor"


# ---- what every case uses -----------------------------------------------------------------------------------------------------------
def _clone(x):
    return x.clone() if torch.is_tensor(x) else tuple(_clone(y) for y in x)


def _same(a, b):
    """torch.equal over (nested tuples of) tensors; float32 by its bits, so that +inf, NaN and the sign of zero count too"""
    if not torch.is_tensor(a):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if a.dtype == torch.float32:
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    return a.shape == b.shape and torch.equal(a, b)


def _alone(calls):
    """every call once on an idle device, each followed by a synchronise and a clone: the warm-up of the case and its expected values"""
    out = []
    for call in calls:
        r = call()
        torch.cuda.synchronize()
        out.append(_clone(r))
    for i in range(len(out)):
        for j in range(i):
            assert not _same(out[i], out[j]), f"calls {j} and {i} give the same result: the case could not see them mixed up"
    return out


def _host_ms(call):
    """host wall time of one undelayed call (after the warm-up), milliseconds"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    call()
    ms = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    return ms


def _delay_for(host_ms):
    """D in whole milliseconds; busy_wait's own check of that length is made here, on an idle device and outside every spy"""
    D = float(round(min(200.0, max(20.0, 10.0 * host_ms))))
    busy_wait(D)
    torch.cuda.synchronize()
    return D


def _back_to_back(calls, D, bypass=False):
    """busy_wait(D), then the calls back to back, each read by an in-stream clone; one synchronise at the end -> (results, records)"""
    with wait_spy(bypass=bypass) as rec:
        busy_wait(D)
        got = [_clone(call()) for call in calls]
        torch.cuda.synchronize()
    return got, rec


def _window(tag, D, host_ms, records, **which):
    n = incomplete(records, **which)
    print(f"[handoffs] {tag}: D = {D:.0f} ms, host {host_ms:.2f} ms per call, {n} of {len(records)} recorded waits found their event incomplete")
    assert n >= 1, (f"INCONCLUSIVE: {tag}: none of the {len(records)} recorded waits {which} found its event incomplete — the device was not "
                    f"late when the host reached the wait, so this run proves nothing about it")
    return n


def _matches(got, want):
    """per result, which of the expected values it equals (for the messages)"""
    return [[j for j, w in enumerate(want) if _same(g, w)] for g in got]


def _under_delay(tag, calls, where):
    """the whole procedure of a case A: expected values one at a time, D from one undelayed call, the delayed run, window proof, equality"""
    want = _alone(calls)
    host = _host_ms(calls[0])
    D = _delay_for(host)
    got, rec = _back_to_back(calls, D)
    _window(tag, D, host, rec, where=where)
    m = _matches(got, want)
    assert m == [[i] for i in range(len(calls))], f"{tag}: result i equals the expected values {m} (should be [[0], [1], [2]])"
    return want, host, D


_FITS = {}


def _hands(tmp_path_factory):
    """two synthetic hand fits at img_size 64 with 7-row motions in which every row's pose and camera differ; the second hand's camera
    is the first's, so that the hands meet (tests/test_gpu_scene_contact.py) -> ((cfg, layer, params, motion), (...))"""
    from harp_amd.playback import Motion
    if not _FITS:
        for seed in (31, 57):
            tmp = tmp_path_factory.mktemp(f"handoff_hand_{seed}")
            _, cfg, layer, params, _ = _setup(T, S, seed, tmp, self_shadow=True, share_light_position=True)
            _FITS[seed] = (cfg, layer, params)
    out = []
    for seed in (31, 57):
        cfg, layer, params = _FITS[seed]
        m = Motion.from_params(params)
        if out:
            m.cam = out[0][3].cam.clone().contiguous()
        out.append((cfg, layer, params, m))
    mA = out[0][3]
    assert len(mA) == T
    for i in range(T):
        for j in range(i):
            assert not torch.equal(mA.pose[i], mA.pose[j]) and not torch.equal(mA.cam[i], mA.cam[j]), (i, j)
    return out


def _avatar(hand, use_graph=True, keep_depth=False):
    from harp_amd.playback import AvatarPlayer
    cfg, layer, params, motion = hand
    p = AvatarPlayer(cfg, params, layer, batch_size=BATCH, ss=1, use_graph=use_graph, device=DEV, keep_depth=keep_depth)
    p.load_motion(motion)
    return p


def _scene(hands, use_graph=True):
    from harp_amd.playback import AvatarPlayer, ScenePlayer
    ps = [AvatarPlayer(cfg, params, layer, batch_size=BATCH, ss=1, use_graph=use_graph, device=DEV, keep_depth=True) for cfg, layer, params, _ in hands]
    scene = ScenePlayer(ps, flip=[False, True])
    scene.load_motions([h[3] for h in hands])
    return scene


def _random_bytes(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n, S, S, 3), generator=g, dtype=torch.uint8).to(DEV)


# ---- A. the players' index table ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
def test_a1_avatar_render_back_to_back(tmp_path_factory, use_graph):
    """AvatarPlayer.render three times behind one busy wait, without and with a staged background: the second call reaches
    idx_done.synchronize() before the first call's upload has run, and must wait there (player.py, _upload)"""
    player = _avatar(_hands(tmp_path_factory)[0], use_graph)
    bg = _random_bytes(4, 1)
    _under_delay(f"A1 render, no background, graph={use_graph}", [lambda r=r: player.render(r) for r in ROWS], "_upload")
    _under_delay(f"A1 render, background, graph={use_graph}", [lambda r=r, b=b: player.render(r, background=bg, bg_rows=b) for r, b in zip(ROWS, SIDE_ROWS)],
                 "_upload")
    assert len(player._graphs) == (2 if use_graph else 0)


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
def test_a2_avatar_flow_back_to_back(tmp_path_factory, use_graph):
    """AvatarPlayer.flow: the only path with a second table, that of the target rows, which has no event of its own — the one wait in
    _upload, in front of both tables, is on the event the previous call's _upload recorded behind both copies"""
    player = _avatar(_hands(tmp_path_factory)[0], use_graph, keep_depth=True)
    _under_delay(f"A2 flow, graph={use_graph}", [lambda r=r, t=t: player.flow(r, t) for r, t in zip(ROWS, TO_ROWS)], "_upload")


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
def test_a3_scene_render_and_contact_back_to_back(tmp_path_factory, use_graph):
    """ScenePlayer over two players: render with a staged scene depth under three different depth_rows, then contact over three
    different row lists"""
    scene = _scene(_hands(tmp_path_factory), use_graph)
    scene.render(ROWS[0])
    torch.cuda.synchronize()
    z = scene.players[0].s["z_c"]
    near, far = float(z[z > 0].min()), float(z[z > 0].max())
    g = torch.Generator().manual_seed(5)                   # no measurement on 20 %, hits and misses around the hands' depths
    depth = ((0.9 * near + (1.1 * far - 0.9 * near) * torch.rand(4, S, S, generator=g)) * (torch.rand(4, S, S, generator=g) > 0.2)).float().to(DEV)
    want, _, _ = _under_delay(f"A3 scene render, scene depth, graph={use_graph}",
                              [lambda r=r, d=d: scene.render(r, scene_depth=depth, depth_rows=d) for r, d in zip(ROWS, SIDE_ROWS)], "_upload")
    plain = scene.render(ROWS[0])
    torch.cuda.synchronize()
    assert not _same(plain, want[0]), "the scene depth must hide something"
    want, _, _ = _under_delay(f"A3 scene contact, graph={use_graph}", [lambda r=r: scene.contact(r) for r in ROWS], "_upload")
    assert all(bool(torch.isfinite(w[5]).any()) for w in want), "the hands must meet"


def test_a1_control_sees_a_table_rewritten_too_early(tmp_path_factory):
    """Positive control: A1 without a background with every Event.synchronize bypassed.  The host then rewrites idx_pin while the first
    upload still sits behind the busy wait, so the first result is no longer its own frames.  All three calls return within a fraction
    of D (D >= 10 x one call), so when the device gets to the FIRST upload the staging buffer already holds the table written LAST:
    the first result is, bit for bit, what the LAST of the calls made behind it should have given.  (The issue that asked for this
    control expected "the second call's frames", which is the outcome of two calls; with the three calls of A1 it is the third's —
    measured on the MI355X: every one of the three results equals the third call's frames.)  The three tables have one length and index one motion: every row on the device is valid."""
    player = _avatar(_hands(tmp_path_factory)[0], True)
    calls = [lambda r=r: player.render(r) for r in ROWS]
    want = _alone(calls)
    host = _host_ms(calls[0])
    D = _delay_for(host)
    got, rec = _back_to_back(calls, D, bypass=True)
    m = _matches(got, want)
    print(f"[handoffs] A1 control: D = {D:.0f} ms, host {host:.2f} ms per call, {incomplete(rec)} of {len(rec)} bypassed waits found their event "
          f"incomplete; result i equals the expected values {m}")
    assert incomplete(rec, where="_upload") >= 1, "INCONCLUSIVE: no bypassed wait found its event incomplete"
    assert not _same(got[0], want[0]), "the control did not see the race"
    assert _same(got[0], want[len(calls) - 1]), m
    got, _ = _back_to_back(calls, D)                         # and with the waits back, right again
    assert _matches(got, want) == [[0], [1], [2]]


# ---- B. _play's pinned frame buffers ------------------------------------------------------------------------------------------------
class _Store:
    """stands in for player._encode: stores (path, array.copy()) after 5 ms, so that futures are still pending when a buffer comes round"""

    def __init__(self):
        self.items, self._lock = [], threading.Lock()

    def __call__(self, path, u8, fmt):
        time.sleep(0.005)
        with self._lock:
            self.items.append((path, u8.copy()))

    def take(self):
        items, self.items = self.items, []
        return items


def _play_case(kind, tmp_path_factory, tmp_path, monkeypatch):
    """(play(out_dir) -> paths, the player whose _run is made late, {file name: expected array}, store, host ms per batch): the warm-up
    play, undelayed, must already store every row's frame (and owner mask) as rendered alone"""
    from harp_amd.playback import player as player_mod
    store = _Store()
    monkeypatch.setattr(player_mod, "_encode", store)
    hands = _hands(tmp_path_factory)
    if kind == "avatar":
        player = _avatar(hands[0])
        play = lambda out: player.play(hands[0][3], str(out), fmt="png")      # noqa: E731
    else:
        player = _scene(hands)
        play = lambda out: player.play([h[3] for h in hands], str(out), fmt="png", masks=True)      # noqa: E731
    n_batches = -(-T // BATCH)
    assert n_batches == 4                                  # each of the two pinned buffers is used twice
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    play(tmp_path / "warm")
    host = (time.perf_counter() - t0) * 1e3 / n_batches
    torch.cuda.synchronize()
    want = {}
    for i in range(T):
        r = player.render([i]) if kind == "avatar" else player.render([i], owner=True)
        torch.cuda.synchronize()
        frames, owner = (r, None) if kind == "avatar" else r
        want["%04d.png" % i] = frames[0].cpu().numpy().copy()
        if owner is not None:
            want["mask_%04d.png" % i] = owner[0].cpu().numpy().copy()
    assert _stored_wrong(store.take(), want) == [], "the undelayed play"
    return play, player, want, store, host


def _stored_wrong(items, want):
    """every path stored exactly once -> the names whose stored array is not the expected one"""
    names = [os.path.basename(p) for p, _ in items]
    assert sorted(names) == sorted(want), (sorted(names), sorted(want))
    return sorted(n for n, (_, a) in zip(names, items) if not (a.shape == want[n].shape and np.array_equal(a, want[n])))


@pytest.mark.parametrize("kind", ["avatar", "scene"])
def test_b_play_with_late_batches(tmp_path_factory, tmp_path, monkeypatch, kind):
    """play() of the 7-row motion in batches of 2 with every batch's device work D late and slow encoders: done.synchronize() must hold
    the host until the batch's frames are in the pinned buffer, before h.numpy() goes to the pool (player.py, _play)"""
    play, player, want, store, host = _play_case(kind, tmp_path_factory, tmp_path, monkeypatch)
    D = _delay_for(host)
    with late_calls(player, "_run", D), wait_spy() as rec:
        play(tmp_path / "late")
        torch.cuda.synchronize()
    assert "_run" not in vars(player)
    _window(f"B play, {kind}", D, host, rec, where="_play")
    wrong = _stored_wrong(store.take(), want)
    assert wrong == [], f"B play, {kind}: stored arrays that are not the row rendered alone: {wrong}"


def test_b_control_sees_frames_taken_too_early(tmp_path_factory, tmp_path, monkeypatch):
    """Positive control: the same with every Event.synchronize bypassed — the encoders get the pinned buffer before the copy into it has
    run.  (The index tables are then rewritten early too: tables of one length over one motion.)  The pinned buffers go back to torch's
    host allocator, which holds them until the copies recorded on them have run; the control ends with a full synchronise."""
    play, player, want, store, host = _play_case("avatar", tmp_path_factory, tmp_path, monkeypatch)
    D = _delay_for(host)
    try:
        with late_calls(player, "_run", D), wait_spy(bypass=True) as rec:
            play(tmp_path / "control")
    finally:
        torch.cuda.synchronize()
    wrong = _stored_wrong(store.take(), want)
    print(f"[handoffs] B control: D = {D:.0f} ms, host {host:.2f} ms per batch, {incomplete(rec, where='_play')} bypassed waits of _play found their "
          f"event incomplete; stored arrays that differ: {wrong}")
    assert incomplete(rec, where="_play") >= 1, "INCONCLUSIVE: no bypassed wait found its event incomplete"
    assert wrong, "the control did not see the race"


# ---- C. the device ingest's staging buffers -----------------------------------------------------------------------------------------
def _ingest_case(tmp_path):
    from harp_amd.utils.data_util import ImagesDataset, ResidentTargets
    rgb, mask = R.make_frames(5, 19, 67, seed=5)
    assert all(not np.array_equal(rgb[i], rgb[j]) and not np.array_equal(mask[i], mask[j]) for i in range(5) for j in range(i))
    ds = ImagesDataset(*R.write_files(tmp_path, rgb, mask), downsample_factor=1)
    host = ResidentTargets(ds)
    ingest = lambda chunk: ResidentTargets(ds, device=DEV, ingest="device", chunk=chunk, workers=2)      # noqa: E731
    ms = {}
    for chunk in (1, 2):                                   # the warm-up: every call of the case once, undelayed
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rt = ingest(chunk)
        ms[chunk] = (time.perf_counter() - t0) * 1e3 / rt.ingest_stats()["chunks"]
        torch.cuda.synchronize()
        assert _ingest_wrong(rt, host) == {}, chunk
    return host, ingest, max(ms.values())


def _ingest_wrong(rt, host):
    """{tensor name: the frames that differ from the host path's}"""
    out = {}
    for name, g, w in zip(("y_true", "y_sil", "y_sil_col"), rt.tensors(), host.tensors()):
        g = g.cpu()
        assert g.shape == w.shape and g.dtype == w.dtype, name
        bad = [i for i in range(w.shape[0]) if not torch.equal(g[i], w[i])]
        if bad:
            out[name] = bad
    return out


def test_c_ingest_with_late_kernels(tmp_path):
    """ResidentTargets(ingest="device") over five frames with every ops.targets_from_u8 D late: with chunk = 1 the copy of chunk k + 1
    sits behind chunk k's delay and has not run when the host comes to decode chunk k + 3 into the same staging buffer —
    free[k & 1].synchronize() must hold it (data_util.py, _ingest_device).  chunk = 2 ends on a short chunk; its three chunks re-use a
    staging buffer once, for a copy that was enqueued before any delay, so a busy wait is also put in front of each ingest: the first
    copies are late too."""
    from harp_amd import ops
    host, ingest, ms = _ingest_case(tmp_path)
    D = _delay_for(ms)
    for chunk in (1, 2):
        with late_calls(ops, "targets_from_u8", D), wait_spy() as rec:
            busy_wait(D)
            rt = ingest(chunk)
            torch.cuda.synchronize()
        _window(f"C ingest, chunk={chunk}", D, ms, rec, where="_ingest_device")
        wrong = _ingest_wrong(rt, host)
        assert wrong == {}, f"C ingest, chunk={chunk}: frames that differ from the host path's: {wrong}"
    assert ops.targets_from_u8.__name__ == "targets_from_u8"


def test_c_control_sees_a_staging_buffer_decoded_into_too_early(tmp_path):
    """Positive control: chunk = 1 with every Event.synchronize bypassed — a later frame of the same size is decoded into a staging
    buffer whose copy has not run"""
    from harp_amd import ops
    host, ingest, ms = _ingest_case(tmp_path)
    D = _delay_for(ms)
    try:
        with late_calls(ops, "targets_from_u8", D), wait_spy(bypass=True) as rec:
            busy_wait(D)
            rt = ingest(1)
    finally:
        torch.cuda.synchronize()
    wrong = _ingest_wrong(rt, host)
    print(f"[handoffs] C control: D = {D:.0f} ms, host {ms:.2f} ms per chunk, {incomplete(rec, where='_ingest_device')} bypassed waits found their "
          f"event incomplete; frames that differ: {wrong}")
    assert incomplete(rec, where="_ingest_device") >= 1, "INCONCLUSIVE: no bypassed wait found its event incomplete"
    assert wrong.get("y_true"), "the control did not see the race"


# ---- D. the monitor's copy stream and slots -----------------------------------------------------------------------------------------
FILL = 0x5A


def _runs_beside_main(stream, ms=5.0):
    """Does work on `stream` run while the main stream is busy?  The runtime spreads its streams over a few hardware queues, and two
    streams on one queue run in order whatever events the code waits for: an event recorded on the idle `stream` behind a busy wait on
    the main stream is complete before that wait is over only if the two can overlap."""
    busy_wait(ms)
    torch.cuda.synchronize()
    e, main = torch.cuda.Event(), torch.cuda.Event()
    busy_wait(ms)
    main.record()
    e.record(stream)
    beside = False
    while not _EVENT_BASE.query(main):                     # (a few milliseconds; not through Event.query: the spy has it)
        beside = beside or _EVENT_BASE.query(e)
    torch.cuda.synchronize()
    return beside


def _monitor_run(base, stacks, D, late, no_wait=False):
    """FitMonitor(slots=1) over the three sheets of stacks[:3], after a first sheet of stacks[3] that makes the monitor create its copy
    stream and its pinned slot (undelayed).  Where that stream cannot overlap the main stream (_runs_beside_main) the monitor is given
    one that can, or neither guard of submit() could be seen missing.  late = "main": a busy wait on the main stream in front of every sheet's producer;
    late = "copy": on the monitor's copy stream in front of every submit; None: no wait.  Every sheet is dropped right after its submit
    and three tensors of its size are allocated and filled on the main stream.  no_wait: the copy stream's wait_event does nothing.
    -> ({name: stored array}, the Event.query records, host ms of the first sheet_u8 + submit)"""
    from harp_amd import ops
    from harp_amd.monitor import FitMonitor
    stored, keep = [], []
    mon = FitMonitor(base, slots=1, encode_fn=lambda path, u8: stored.append((os.path.basename(path), u8.copy())))
    cs = None
    try:
        with wait_spy(method="query") as rec:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            mon.submit("first.jpg", ops.sheet_u8(stacks[3]))
            host = (time.perf_counter() - t0) * 1e3
            cs = mon._copy_stream
            beside = [_runs_beside_main(cs)]
            while not beside[-1] and len(beside) < 9:      # the monitor's stream shares the main stream's queue: one that does not
                cs = mon._copy_stream = torch.cuda.Stream()
                beside.append(_runs_beside_main(cs))
            print(f"[handoffs] D monitor: copy stream runs beside the main stream: {beside}")
            assert beside[-1], "INCONCLUSIVE: no stream was found that runs beside the main stream; the copy can never be ahead or behind"
            if no_wait:
                cs.wait_event = lambda event: None
            for k in range(3):
                if late == "main":
                    busy_wait(D)
                elif late == "copy":
                    with torch.cuda.stream(cs):
                        busy_wait(D)
                sheet = ops.sheet_u8(stacks[k])
                n = sheet.numel()
                mon.submit("sheet%d.jpg" % k, sheet)
                del sheet
                keep += [torch.full((n,), FILL, dtype=torch.uint8, device=DEV) for _ in range(3)]
            mon.close()
    finally:
        if cs is not None and "wait_event" in vars(cs):
            del cs.wait_event
        mon.close()
        torch.cuda.synchronize()
    names = [n for n, _ in stored]
    assert sorted(names) == ["first.jpg", "sheet0.jpg", "sheet1.jpg", "sheet2.jpg"], names
    return dict(stored), rec, host


def _monitor_case(tmp_path):
    from harp_amd import ops
    g = torch.Generator().manual_seed(9)
    stacks = torch.rand(4, 9, S, S, 3, generator=g).to(DEV)
    want = {}
    for k in range(3):
        sheet = ops.sheet_u8(stacks[k])
        torch.cuda.synchronize()
        want["sheet%d.jpg" % k] = sheet.cpu().numpy().copy()
        sheet.fill_(FILL)                                  # (the block goes back to the allocator without the picture)
        del sheet
    assert not any(np.array_equal(want["sheet%d.jpg" % i], want["sheet%d.jpg" % j]) for i in range(3) for j in range(i))
    got, _, host = _monitor_run(str(tmp_path / "warm") + "/", stacks, 0.0, None)      # the warm-up: every call once, undelayed
    assert _sheets_wrong(got, want) == [], "the undelayed monitor"
    # the warm-up's sheets went back to the allocator as they were, and the same sequence of allocations hands a sheet the block it had
    # before: every free block of a sheet's size is overwritten, so that a copy that runs ahead of its producer cannot find the picture
    poison = [torch.full((want["sheet0.jpg"].size,), FILL, dtype=torch.uint8, device=DEV) for _ in range(64)]
    torch.cuda.synchronize()
    del poison
    return stacks, want, host


def _sheets_wrong(got, want):
    return sorted(n for n, w in want.items() if not (got[n].shape == w.shape and np.array_equal(got[n], w)))


@pytest.mark.parametrize("late", ["main", "copy"])
def test_d_monitor_with_a_late_producer_or_copy(tmp_path, late):
    """late = "main": the sheet's producer is D late, the copy stream must wait for the event recorded behind it (cs.wait_event(ready)).
    late = "copy": the copy is D late while the sheet is dropped and its size allocated and filled three times on the main stream:
    the sheet's block must not be handed out before the copy has read it (sheet.record_stream(cs)).  The writer thread must not read
    the pinned slot before the copy's event is complete, and with one slot the next submit waits for the writer."""
    stacks, want, host = _monitor_case(tmp_path)
    D = _delay_for(host)
    got, rec, _ = _monitor_run(str(tmp_path / late) + "/", stacks, D, late)
    _window(f"D monitor, late {late} stream", D, host, rec, thread=WRITER)
    wrong = _sheets_wrong(got, want)
    assert wrong == [], f"D monitor, late {late} stream: stored sheets that are not ops.sheet_u8 of their stack: {wrong}"


def test_d_control_sees_a_copy_ahead_of_its_producer(tmp_path):
    """Positive control: late = "main" with the copy stream's wait_event replaced by a no-op — the copy reads the sheet's own allocated
    block before the producer has written it (a valid read of memory the test owns)"""
    stacks, want, host = _monitor_case(tmp_path)
    D = _delay_for(host)
    got, rec, _ = _monitor_run(str(tmp_path / "control") + "/", stacks, D, "main", no_wait=True)
    wrong = _sheets_wrong(got, want)
    print(f"[handoffs] D control: D = {D:.0f} ms, host {host:.2f} ms per call; stored sheets that differ: {wrong}")
    assert wrong, "the control did not see the race"
