"""The host side of a device-resident sampling chain, shared by every process: the chain's device tables, the recorder of its frames,
the one host walk "frame, step, frame ... last frame", the one capture of a launch sequence into a hipGraph, and `ChainRunner`, the
replayable step.  The processes (ddpm.py and the samplers built on it) supply the tables and the C call of their kind."""

from __future__ import annotations

import gc
from typing import Optional

import torch
from torch import Tensor

from .. import _lib
from ..common import vis
from ..common.noise import philox_reserve


class ChainTables:
    """the device side of a chain (include/dmme_hip.h: dmme_chain_*): the per-index scalars of the update `coef` [n+1][4], the
    timestep at each loop index `ttab`, and the 64-byte loop `state` {i, t, Philox offset, seed, ticket}"""

    def __init__(self, rows, ttab, device):
        self.coef = torch.tensor(rows, dtype=torch.float32).reshape(-1).to(device)
        self.ttab = torch.tensor(ttab, dtype=torch.int64).to(device)
        self.state = torch.zeros(8, dtype=torch.int64, device=device)

    def set(self, i: int, seed: int = 0, offset: int = 0):
        """place the loop at index i (DDPM: t = i) with the Philox stream at (seed, offset in quads)"""
        _lib.check(_lib.lib().dmme_chain_set(_lib.ptr(self.state), int(i), _lib.ptr(self.ttab), seed & 0xFFFFFFFFFFFFFFFF, int(offset), _lib.stream_ptr()), "dmme_chain_set")


ROW_DRAWS = {}  # kind -> does a step over this table row read normals?  Each conditioned sampler states its rule beside its row layout and enters it here


def chain_draws(kind: int, rows) -> bool:
    """does a chain of this kind over these table rows consume normals?  The host's statement of the kernels' noise rule (csrc/common.h:
    kind_noise): the shipped DDIM kinds and DPM-Solver++ never do, the paper-form DDIM kinds only with a non-zero k2 somewhere, DDNM and
    DPS where a row draws (`ROW_DRAWS`), every kind with a DDPM mean does, and so do RePaint and ILVR whatever their rows say.  A chain
    that draws nothing leaves torch's generator where the eager loop leaves it."""
    if kind in (_lib.CHAIN_DDIM, _lib.CHAIN_DDIM_GUIDED, _lib.CHAIN_DPMPP, _lib.CHAIN_DPMPP_CFG):
        return False
    if kind in (_lib.CHAIN_GDDIM, _lib.CHAIN_GDDIM_CFG):
        return any(r[2] != 0.0 for r in rows)
    if kind in (_lib.CHAIN_DDNM, _lib.CHAIN_DPS):
        return any(ROW_DRAWS[kind](r) for r in rows)
    if kind == _lib.CHAIN_PFODE:  # (w of the likelihood's trace term: a stage that carries one draws a Rademacher probe)
        return any(r[4] != 0.0 for r in rows)
    return True


def history_ordinals(count: int, vis_length: int):
    """the step ordinals after which a chain of `count` steps keeps a frame (0: before the first step), `vis_length` of them where the
    chain is long enough.  With count = T this is the reference's `save_t` and its final append (callbacks/generate.py:73-84): a frame
    in front of the step from t = int(T / (L-1) * i) is a frame after T - t steps.  Ordinals, not timesteps: RePaint's index is not monotone."""
    count, L = int(count), int(vis_length)
    if count < 0 or L < 1:
        raise ValueError(f"history_ordinals: count = {count} steps, vis_length = {L}")
    return sorted({count - int(count / (L - 1) * i) for i in range(L - 1, 0, -1)} | {count})


class HistoryRecorder:
    """The frames of one chain as a grid on the device: a canvas allocated and zeroed once, and per kept frame ONE dmme_grid_tile launch
    (denorm + placement, as float32 or as uint8) on the chain's stream - no allocation, no synchronisation, no copy to the host while
    the chain runs.  Image b of frame k sits in row b, column k (cell k + b * len(ordinals)), which is what `make_history` builds from
    the list of denormed frames the reference's callback collects; with a single ordinal the images are laid out as `make_history`
    lays out a single history.  `canvas` is read after the chain; a later chain overwrites every cell.  `recorded`: frames of the last chain."""

    def __init__(self, n_images: int, C: int, H: int, W: int, ordinals, out_kind: int = 0, device="cuda"):
        self.ordinals = sorted({int(s) for s in ordinals})
        if n_images < 1 or not self.ordinals or self.ordinals[0] < 0:
            raise ValueError(f"HistoryRecorder: {n_images} images, ordinals {self.ordinals}")
        self.n_images, self.image = int(n_images), (int(C), int(H), int(W))
        L = self.stride = len(self.ordinals)
        if L == 1:
            self.xmaps = min(vis.history_nrow(self.n_images), self.n_images)
            self.ymaps = -(-self.n_images // self.xmaps)
        else:
            self.xmaps, self.ymaps = L, self.n_images
        self.pad = 0 if L * self.n_images == 1 else vis.PAD  # (make_grid returns a batch of one image unpadded)
        self.canvas = vis.new_canvas(*self.image, self.xmaps, self.ymaps, self.pad, out_kind, device)
        self._slot = {s: k for k, s in enumerate(self.ordinals)}
        self.recorded = 0

    def begin(self, x: Tensor, count: int) -> None:
        """a chain of `count` steps on the buffer `x` starts: refuses what would leave a cell unwritten or write outside the canvas"""
        if tuple(x.shape[1:]) != self.image or x.shape[0] < self.n_images or x.device != self.canvas.device:
            raise ValueError(f"HistoryRecorder: built for {self.n_images} images of {self.image} on {self.canvas.device}, the chain runs on {tuple(x.shape)} on {x.device}")
        if self.ordinals[-1] > count:
            raise ValueError(f"HistoryRecorder: ordinal {self.ordinals[-1]} in a chain of {count} steps")
        self.recorded = 0

    def at(self, s: int, x: Tensor) -> None:
        """`s` steps are done and `x` holds their result: keep its first n_images images if that frame is wanted"""
        k = self._slot.get(s)
        if k is not None:
            vis.grid_tile(x[: self.n_images], self.canvas, k, self.stride, self.xmaps, self.ymaps, self.pad)
            self.recorded += 1


def walk(x: Tensor, first: int, count: int, step, recorder=None, reserve=None) -> Tensor:
    """THE host loop of a chain, eager or replayed: `step(s, i)` for the ordinals s = 0 .. count - 1 at the loop indices i = first - s,
    in place on `x`.  A `recorder` is asked first (`begin`: it refuses a chain it does not fit before anything is drawn or launched),
    sees x in front of every step (`at(s, x)`) and once behind the last (`at(count, x)`); a walk of no steps records frame 0 only.
    `reserve()`: called once between `begin` and the first step, where a chain takes its span of the Philox stream - a refused
    recorder leaves torch's generator where it was."""
    if recorder is not None:
        recorder.begin(x, count)
    if reserve is not None:
        reserve()
    for s in range(count):
        if recorder is not None:
            recorder.at(s, x)
        step(s, first - s)
    if recorder is not None:
        recorder.at(count, x)
    return x


def eager_chain(x: Tensor, kind: int, tables, first: int, streams: int, call, history=None) -> Tensor:
    """THE eager host loop of a conditioned sampler, in place on x: `first` steps from loop index `first` down over `tables`, each
    `call(row, t, z)` with the table row, the timestep as a (1,) device tensor and the step's normals ([streams][numel], None where
    `ROW_DRAWS[kind]` says the row reads none).  The normals come from dmme_randn at the offsets the captured chain's state walks through,
    so the two agree bit for bit under the same seed; the span is taken where the chain's runner takes it (`chain_draws`), once the
    recorder has accepted the walk."""
    n, rows, ttab = tables
    numel, row_draws = x.numel(), ROW_DRAWS[kind]
    span = []
    tt = torch.tensor(ttab, dtype=torch.int64, device=x.device).unsqueeze(1)
    z = torch.empty(streams * numel, dtype=torch.float32, device=x.device)

    def step(k, i):
        draws = row_draws(rows[i])
        if draws:
            _lib.check(_lib.lib().dmme_randn(_lib.ptr(z), z.numel(), span[0], span[1] + k * streams * (numel // 4), _lib.stream_ptr()), "dmme_randn")
        call(rows[i], tt[i], z if draws else None)

    return walk(x, first, first, step, history, lambda: span.extend(philox_reserve(x.device, streams * numel * first) if chain_draws(kind, rows) else (0, 0)))


def capture(launch, check, carried=()):
    """`launch()` (a fixed sequence of kernel launches on fixed buffers) as a hipGraph: (graph, what launch() returned inside the
    capture, None), or (None, None, the capture's RuntimeError) - what a failed capture means is the caller's decision.

    One eager trial launch comes first (weight packing and kernel attribute setup happen at a first launch), then a device
    synchronisation and `check()`, the level engine's status word.  The trial is OUTSIDE the fallback: a DmmeError, a hand-off timeout
    or a kernel fault in it is a real error and propagates, leaving the caller with no graph and no "capture failed" mark; only a
    failure of the CAPTURE itself (stream capture unavailable / invalidated) is handed back, and the caller then issues the same
    launches eagerly.  `carried`: the buffers a launch changes and the next one reads; the trial and the capture leave them as found."""
    saved = [b.clone() for b in carried]

    def restore():
        for b, v in zip(carried, saved):
            b.copy_(v)

    launch()
    torch.cuda.synchronize()
    check()
    restore()
    graph, out, error = None, None, None
    # No finalizer may run inside the capture: a dropped network's plan frees its device tables, a dropped runner's graph gives back its
    # memory pool - device-memory calls the capture forbids - and torch's capture no longer collects garbage on entry, so Python's
    # automatic collector could pick any allocation inside `launch()` to run them.  Collect now; keep the collector off until the
    # capture has ended.
    gc.collect()
    gc_was_on = gc.isenabled()
    gc.disable()
    try:
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = launch()
    except RuntimeError as exc:
        graph, out, error = None, None, exc
    finally:
        if gc_was_on:
            gc.enable()
    restore()
    return graph, out, error


class ChainRunner(ChainTables):
    """One replayable denoising step on a fixed image buffer (include/dmme_hip.h: dmme_chain_*).

    The loop state (index i, timestep t, Philox seed / offset) and the per-index scalars of the update live on the device;
    `step()` replays ONE captured hipGraph of  time MLP + UNet + noise draw + sampler update + state advance  - no host value
    changes between steps, nothing is copied host-to-device, nothing synchronises.  `x` is updated in place.  Falls back to
    issuing the same launches eagerly when graph capture is unavailable (same results either way)."""

    def __init__(self, process, x: Tensor, use_graph: bool = True, spec=None):
        """`spec`: an explicit (kind, (n, rows, t_table)) in place of the process's own `_chain_kind` / `_chain_tables()` - a process
        with more than one chain over the same network (GeneralizedDDIM: the reversed tables of its encoding direction)"""
        model = process.model
        if not (isinstance(x, Tensor) and x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 4):
            raise ValueError("ChainRunner needs a contiguous fp32 GPU image batch")
        B, _, H, W = x.shape
        self.process, self.model, self.x = process, model, x
        self.plan = model._plan_for(B, H, W, x.device)
        self.kind, (n, rows, ttab) = spec if spec is not None else (process._chain_kind, process._chain_tables())
        self.draws = chain_draws(self.kind, rows)
        self.n_steps = n
        self.pred = getattr(process, "_pred", _lib.PRED_EPS)
        self.pred_ab = process._pred_table(x.device).clone() if self.pred != _lib.PRED_EPS else None  # (the runner's own: see _set_prediction)
        # x0 thresholding: the process's setting when the runner is built (`_runner_key` holds it), its table and the streaming form's
        # scratch held by this runner because the captured graph holds their addresses
        self.thr = getattr(process, "_thr", _lib.THRESHOLD_NONE)
        self.thr_tab, self.thr_scratch, self.thr_k, self.thr_frac = None, None, 0, 0.0
        if self.thr != _lib.THRESHOLD_NONE:
            from .ddpm import threshold_rank

            self.thr_tab = process._thr_table(x.device).clone()
            if self.thr == _lib.THRESHOLD_DYNAMIC:
                self.thr_k, self.thr_frac = threshold_rank(process.threshold_percentile, x[0].numel())
                self.thr_scratch = torch.empty(int(_lib.lib().dmme_x0_threshold_scratch_bytes(B, x[0].numel())) // 4, dtype=torch.int32, device=x.device)
        super().__init__(rows, ttab, x.device)
        self.out =torch.empty((B, model.out_channels, H, W), dtype=torch.float32, device=x.device)
        self.quads = x.numel() // 4
        self.noise_numel = x.numel()  # normals one step consumes (a runner whose buffer holds more than the images it draws for says so)
        self.use_graph = use_graph
        self.graph = None
        self.capture_error = None  # why this runner launches eagerly although a graph was asked for (None: it does not)
        self._wkey = None

    def _set_prediction(self, plan=None):
        """tell the plan what its network predicts, in front of every chain-step call: the plan is shared by every process that wraps
        the same network, so an eps process says so too.  `pred_ab` is the process's device table, held by this runner because the
        captured graph holds its address."""
        plan = self.plan if plan is None else plan
        _lib.check(_lib.lib().dmme_unet_plan_set_prediction(plan.h, self.pred, _lib.ptr(self.pred_ab), self.process.timesteps), "dmme_unet_plan_set_prediction")

    def no_threshold(self):
        """this runner's chain never clips (GeneralizedDDIM's encoding direction: clipping would break the inversion)"""
        self.thr = _lib.THRESHOLD_NONE
        return self

    def _set_threshold(self, plan=None):
        """tell the plan how its eps prediction is thresholded, in front of every chain-step call, for the reason `_set_prediction` is"""
        plan = self.plan if plan is None else plan
        _lib.check(_lib.lib().dmme_unet_plan_set_threshold(plan.h, self.thr, _lib.ptr(self.thr_tab), self.process.timesteps, self.thr_k, self.thr_frac,
                                                           _lib.ptr(self.thr_scratch)), "dmme_unet_plan_set_threshold")

    def _launch(self, packed):
        """the launches of one step, eager or under capture; a subclass supplies `_call`, the entry point of its kind"""
        self._set_prediction()
        self._set_threshold()
        self._call(packed)
        self.plan.overwritten()

    def _call(self, packed):
        _lib.check(
            _lib.lib().dmme_chain_step(self.plan.h, _lib.ptr(packed), _lib.ptr(self.x), _lib.ptr(self.out), _lib.ptr(self.plan.workspace), self.kind,
                                       _lib.ptr(self.coef), _lib.ptr(self.ttab), _lib.ptr(self.state), _lib.stream_ptr()),
            "dmme_chain_step",
        )

    def _carried(self):
        """the buffers a step changes and the next step reads: what the trial step and the capture must leave as they found it"""
        return [self.x, self.state]

    def _weights_key(self):
        """identifies the packed weights the captured graph reads"""
        return (self.plan.packed_version, self.plan.fold_version, self.plan.packed.data_ptr())

    def _packed(self):
        """the packed weights the step's forward reads, brought up to date outside any capture: the no-grad form's, re-packed (and the
        attention blocks re-folded) when the parameters changed.  A runner whose step keeps the forward's context for a backward
        (PosteriorChainRunner) hands over the unfolded weights and the backward's buffers instead."""
        return self.model._packed_for(self.plan, fold=True)

    def step(self):
        model = self.model
        if model.training:
            raise RuntimeError("ChainRunner: sampling chains run in eval mode (no dropout masks inside the replayed step)")
        packed = self._packed()
        wkey = self._weights_key()
        if not self.use_graph or self.capture_error is not None:
            self._launch(packed)
            return self.x
        if self.graph is None or self._wkey != wkey:
            # (see `capture`: an error of its trial step propagates; a failed capture makes this runner, not the model, stay eager)
            self.graph, _, self.capture_error = capture(lambda: self._launch(packed), self.plan.check, self._carried())
            if self.graph is None:
                self._launch(packed)
                return self.x
            self._wkey = wkey
        # (no synchronisation while the engine's status word is clear: an atomic load of pinned host memory; a hand-off timeout of an
        # earlier replayed step raises here, one step late at most, for callers that never reach `run`'s final check)
        self.plan.check()
        self.graph.replay()
        self.plan.overwritten()
        return self.x

    def run(self, first: int, count: int, recorder: Optional[HistoryRecorder] = None):
        """`count` steps from loop index `first` downwards, drawing from torch's CUDA generator like the eager loop.  `recorder`: the
        frames it wants (keyed on the number of steps done) go to its canvas, one launch each on this stream between two replays."""

        def reserve():
            seed, off = philox_reserve(self.x.device, self.noise_numel * count) if self.draws else (0, 0)
            self.set(first, seed, off)

        walk(self.x, first, count, lambda s, i: self.step(), recorder, reserve)
        # replayed graphs do not pass through the C entry points that look at the level engine's status word: one synchronisation
        # per chain (the caller reads the images next anyway), then the check - a chain never returns numbers from a launch that
        # gave up on a hand-off (DmmeError instead)
        torch.cuda.current_stream(self.x.device).synchronize()
        self.plan.check()
        return self.x

    _side = ()  # the fixed buffers a subclass keeps beside x (read only: a chain fills them once), by attribute name

    def run_copies(self, x: Tensor, side, first: int, recorder: Optional[HistoryRecorder] = None) -> Tensor:
        """the chain from loop index `first` down to 0 on copies of x and of `side`, one tensor per name in `_side`; a new tensor"""
        self.x.copy_(x)
        for name, v in zip(self._side, side):
            getattr(self, name).copy_(v)
        return self.run(first, first, recorder).clone()


class KeepForwardRunner(ChainRunner):
    """a ChainRunner whose step keeps the forward's context for an input-only backward (DPS, the likelihood's stage): it hands over the
    UNFOLDED weights (the keep form never reads the folded attention matrices) and, beside them, the backward's workspace and
    data-gradient weights, brought up to date outside any capture"""

    def _packed(self):
        return self.model._bwd_buffers(self.plan)

    def _weights_key(self):
        p = self.plan
        return super()._weights_key() + (p.packed_bwd_version, p.packed_bwd.data_ptr(), p.bws.data_ptr())
