"""Continuous batching for the sampler: a queue whose engine rows are SLOTS, refilled the tick after a chain ends.

Every other entry point (`model(x, image)`, `predict_multiple`, the evaluators) is a closed call: the batch is fixed when the call starts
and all its samples walk the same rows in lockstep.  A service that gets 1-16 samples of one image at a time, with walks of different
lengths, then runs the chip at a fraction of its batch-64 rate.  `SamplingQueue` keeps ONE engine of `capacity` rows busy instead:

    q = SamplingQueue(model, capacity=64, image_shape=(C, H, W))      # or model.sampling_queue(...)
    r = q.submit(condition, x=None, t=None, vote=None)                # any number of requests, at any time
    q.step(ticks=1); q.run_until_idle()
    r.done; r.result()["diffusion_out"]                               # what model(x, condition, t=t) returns

The construction.  Every network kernel reads its time-embedding row as rowmap[n] + step, so one network pass can hold samples at
different noise levels; the pass stops at x0 (every table row has mode STEP_SOFTMAX_ONLY, as in a guided call) and ONE launch behind it,
ccdm_slots_step, does the reverse step of every slot with that slot's own coefficients, mode, step row, Philox key and global sample
index, read from a device table of one hip.SlotRow per slot (include/ccdm_hip.h has the definition).  One tick is: the admissions
(SamplerEngine.set_slot_inputs), the upload of rowmap and the slot table, the network pass, the slots' step, and for every slot whose
walk ended a device-to-device copy of its result into the request's own tensor — all enqueued on the engine's stream, no host
synchronisation.  Which sample sits in which slot at which tick is decided by the pure functions below (`plan_walk`, `schedule_tick`,
`slot_rows`, `simulate`), which need no device.

The contract.  Whatever the arrival schedule and whatever else is in flight, r.result()["diffusion_out"] is torch.equal to what
model(x, condition, t=t) returns in a fresh solo call with `philox_call` set to the request's call index and `step_T_sample` to its vote
— class maps and "confidence" probabilities alike: a request IS a call (it takes the key of the current `philox_call` and advances the
counter as a call does), sample j of it is global sample model.sample_offset + j, and the draw is keyed by (pixel, global sample, row of
the request's own walk), never by the slot.  Its limits: it holds wherever a sample's bits in the network pass do not depend on the
batch — the default slicing = "throughput" (with "latency" the slice rule depends on the batch size: the queue is self-consistent, and
equal to a solo call only where that call's batch takes the same rule as `capacity` does, DenoisingModel._fine_slices).  The one kernel
choice that looks at the batch size, ccdm_attention's 4 or 8 waves per block for sequences of 2048 tokens and more, changes no result
bit (every wave owns its queries and walks the same key tiles in the same order), so it is inside the contract.

Range overflow.  The engine's range flag is one per engine; it is copied next to every finished sample's result.  A set flag fails that
request and every later one with hip.CcdmRangeError until `reset()`, which clears the flag and drops what is in flight.  There is no
automatic fp32 re-run: the caller sets model.prec = hip.PREC_F32 (or pins layers in model.f32_layers) and resubmits.

Guided requests.  SamplingQueue(..., guided=True) takes requests with the guidance of an annotator in the loop,

    q = model.sampling_queue(64, (C, H, W), guided=True)
    r = q.submit(condition, evidence=e, known_labels=y, temperature=0.7, truncation=0.9)          # any subset, or none

checked by a solo call's own guidance.check_guidance, with a solo call's meaning and errors.  The tick's
step is then ccdm_slots_guided_step: beside the slot table a second one of one hip.SlotGuideRow per slot — the shaping, the clamp's
(p_hit, p_miss) of the slot's row (`plan_clamp`), two flags — filled by `slot_guide_rows`, and two slot-indexed pools in the engine
(evidence, known labels) that an admission fills (SamplerEngine.set_slot_guidance) from the request's own device copies.  Per slot the
launch does what a solo call's run_row does behind the network pass: evidence multiply, shaping, step, clamp.  The contract is the
same: the result is torch.equal to model(x, condition, t=t, evidence=..., known_labels=..., temperature=..., truncation=...) under the
request's call index and vote, whatever else — guided or not — is in flight.  A queue built without guided=True is the plain queue,
launch for launch, and refuses every guidance keyword.

Not thread-safe: the caller drives `step`.  Not built: `views`, `tiles` and `resample` in a queue (several engine rows per sample; a
walk that revisits rows), evidence that changes from pass to pass, feature_condition."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import guidance as G
from . import hip
from .guidance import GUIDANCE_KEYWORDS  # noqa: F401  (its home is guidance.py; the name stays readable here)
from .models import DenoisingModel, OneHotCategoricalBCHW, step_values

# one row of ccdm_slots_step's table as numpy sees it (hip.SlotRow: 32 bytes)
SLOT_DTYPE = np.dtype([("alpha_t", "<f4"), ("cumalpha_tm1", "<f4"), ("mode", "<i4"), ("step_row", "<i4"), ("key_lo", "<u4"), ("key_hi", "<u4"),
                       ("sample", "<u4"), ("reserved", "<u4")])

# one row of ccdm_slots_guided_step's second table (hip.SlotGuideRow: 32 bytes)
GUIDE_DTYPE = np.dtype([("inv_temperature", "<f4"), ("top_r", "<f4"), ("p_hit", "<f4"), ("p_miss", "<f4"), ("flags", "<i4"), ("reserved", "<i4", (3,))])

# what a request of a guided queue takes, and why it takes no other
QUEUED_GUIDANCE = ("evidence", "known_labels", "temperature", "truncation")
NOT_QUEUED = {"views": "a sample with views is several engine rows", "tiles": "a tiled sample is several engine rows",
              "resample": "a walk with resampling jumps visits rows more than once"}
# a request's guidance as the scheduler's pure functions see it: (inv_temperature, top_r, has evidence, the clamp pair of every row of
# its walk or None)
Guide = Tuple[float, float, bool, Optional[List[Tuple[np.float32, np.float32]]]]

# a walk: per row (emb row, alpha_t, cumalpha_tm1, mode); the row's index is its step_row
Walk = List[Tuple[int, float, float, int]]
# the scheduler's state: per slot None or (request id, sample index in the request, next row of its walk); the waiting samples, first in first out
Slots = Tuple[Optional[Tuple[int, int, int]], ...]
Pending = Tuple[Tuple[int, int], ...]


# ------------------------------------------------------------------------------------------------------------------ pure scheduling
def last_mode_of(vote: Optional[str]) -> int:
    """The mode of a walk's row at t = 1, by _forward_denoising's rule."""
    return (hip.STEP_LAST_MAJORITY if vote is None or vote == "majority"
            else hip.STEP_LAST_CONFIDENCE if vote == "confidence" else hip.STEP_LAST_KEEP)


def plan_walk(time_steps: int, init_t: Optional[int], vote: Optional[str], posterior_coeffs) -> Walk:
    """A request's walk: step_values(T, t) with posterior_coeffs, row j = (emb row T - t_j of the all-levels table, alpha_t,
    cumalpha_tm1, STEP_SAMPLE above t = 1 and the vote's mode at it) — a walk that stops above t = 1 ends in a STEP_SAMPLE row."""
    last = last_mode_of(vote)
    walk = []
    for t in step_values(time_steps, init_t):
        a, c = posterior_coeffs(t)
        walk.append((time_steps - t, float(a), float(c), hip.STEP_SAMPLE if t > 1 else last))
    return walk


def schedule_tick(slots: Slots, pending: Pending, walk_len: Dict[int, int]):
    """One tick's decisions, nothing mutated: the free slots in ascending order take the waiting samples first in, first out; every
    occupied slot then runs the next row of its sample's walk; a sample whose walk ends leaves its slot free for the next tick.
    Returns (slots', pending', admitted, active, finished): admitted = [(slot, request, sample)], active = [(slot, request, sample,
    row)] in slot order, finished = [(slot, request, sample)]."""
    cur = list(slots)
    wait = list(pending)
    admitted = []
    for s, held in enumerate(cur):
        if not wait:
            break
        if held is None:
            req, j = wait.pop(0)
            cur[s] = (req, j, 0)
            admitted.append((s, req, j))
    active, finished = [], []
    for s, held in enumerate(cur):
        if held is None:
            continue
        req, j, row = held
        active.append((s, req, j, row))
        if row + 1 == walk_len[req]:
            finished.append((s, req, j))
            cur[s] = None
        else:
            cur[s] = (req, j, row + 1)
    return tuple(cur), tuple(wait), admitted, active, finished


def slot_rows(capacity: int, active: Sequence[Tuple[int, int, int, int]], walks: Dict[int, Walk], keys: Dict[int, int],
              sample0: Dict[int, int], rowmap: Optional[np.ndarray] = None, table: Optional[np.ndarray] = None):
    """The two uploads of a tick from its active list: rowmap int32 [capacity] (the emb row of every slot's network pass; an idle slot
    runs row 0) and the slot table SLOT_DTYPE [capacity] (idle slots marked hip.SLOT_IDLE).  keys[request] = the request's Philox key,
    sample0[request] = the global index of its sample 0.  Written into `rowmap` / `table` where given (pinned buffers)."""
    rowmap = np.zeros(capacity, np.int32) if rowmap is None else rowmap
    table = np.zeros(capacity, SLOT_DTYPE) if table is None else table
    rowmap[:] = 0
    table[:] = np.zeros((), SLOT_DTYPE)
    table["mode"] = hip.SLOT_IDLE
    for s, req, j, row in active:
        emb, a, c, mode = walks[req][row]
        rowmap[s] = emb
        table[s] = (a, c, mode, row, keys[req] & 0xFFFFFFFF, (keys[req] >> 32) & 0xFFFFFFFF, (sample0[req] + j) & 0xFFFFFFFF, 0)
    return rowmap, table


def plan_clamp(walk: Walk, K: int) -> List[Tuple[np.float32, np.float32]]:
    """Per row of a walk the clamp's (p_hit, p_miss) as SamplerEngine.clamp_known_labels forms it: c + (1 - c) / K and (1 - c) / K in
    float64, each rounded to fp32 once; c = the row's cumalpha_tm1, and 1.0 on the walk's last row (the labels themselves)."""
    pairs = []
    for j, (_, _, c, _) in enumerate(walk):
        c = 1.0 if j == len(walk) - 1 else float(c)
        p_miss = (1.0 - c) / K
        pairs.append((np.float32(c + p_miss), np.float32(p_miss)))
    return pairs


def slot_guide_rows(capacity: int, active: Sequence[Tuple[int, int, int, int]], guides: Dict[int, Guide], table: Optional[np.ndarray] = None):
    """The third upload of a guided queue's tick from its active list: the guide table GUIDE_DTYPE [capacity].  guides[request] = the
    request's Guide; a request without an entry, and every idle slot, gets the neutral row (1, 1, 0, 0, flags 0).  Written into `table`
    where given (a pinned buffer)."""
    table = np.zeros(capacity, GUIDE_DTYPE) if table is None else table
    table[:] = np.zeros((), GUIDE_DTYPE)
    table["inv_temperature"] = 1.0
    table["top_r"] = 1.0
    for s, req, j, row in active:
        if req not in guides:
            continue
        inv_t, top_r, has_evidence, clamp = guides[req]
        p_hit, p_miss = clamp[row] if clamp is not None else (0.0, 0.0)
        flags = (hip.SLOT_GUIDE_EVIDENCE if has_evidence else 0) | (hip.SLOT_GUIDE_KNOWN if clamp is not None else 0)
        table[s] = (inv_t, top_r, p_hit, p_miss, flags, (0, 0, 0))
    return table


def simulate(capacity: int, arrivals: Sequence[Tuple[int, int, int, int]]):
    """Run the scheduler without a device.  arrivals: (tick, request id, n, walk length), submitted before that tick in the order
    listed.  Ticks run until nothing is held or waiting or still to arrive.  Returns the ticks as a list of (admitted, active, finished)."""
    slots: Slots = (None,) * capacity
    pending: Pending = ()
    walk_len: Dict[int, int] = {}
    todo = sorted(arrivals, key=lambda a: a[0])          # (stable: the listed order within a tick)
    ticks = []
    tick = 0
    while todo or pending or any(h is not None for h in slots):
        while todo and todo[0][0] <= tick:
            _, req, n, length = todo.pop(0)
            walk_len[req] = length
            pending = pending + tuple((req, j) for j in range(n))
        slots, pending, admitted, active, finished = schedule_tick(slots, pending, walk_len)
        ticks.append((admitted, active, finished))
        tick += 1
    return ticks


# ------------------------------------------------------------------------------------------------------------------ the queue
class QueueRequest:
    """What `submit` returns.  `done`: every sample's walk has been enqueued to its end (the device may still be running it);
    `result()`: the output of the equivalent solo call — it drives the queue until the request is done if it is not, then waits for the
    device, and raises hip.CcdmRangeError if the engine's range flag was set when a sample of the request finished."""

    def __init__(self, queue: "SamplingQueue", rid: int, n: int, call: int, key: int, sample0: int, vote: Optional[str], walk: Walk,
                 init_t: Optional[int], out_device: torch.device):
        self.queue, self.id, self.n, self.call, self.key, self.sample0, self.vote, self.walk = queue, rid, n, call, key, sample0, vote, walk
        self.init_t, self.out_device = init_t, out_device
        self.finished = 0
        self.dropped = False
        self.cond: Optional[torch.Tensor] = None          # device copies, held until every sample has been admitted and has run
        self.xt_idx: Optional[torch.Tensor] = None
        self.guide: Optional[Guide] = None                # a guided request's table values, and its maps on the device (held like cond)
        self.ev: Optional[torch.Tensor] = None            # fp32 [n,H*W,K]
        self.known: Optional[torch.Tensor] = None         # uint8 [n,H*W]
        self.buf: Optional[torch.Tensor] = None           # the result rows: [n,H,W,K] fp32 / int64, or [n,H*W] uint8 class indices
        self.flag: Optional[torch.Tensor] = None          # the engine's range flag as it stood behind the last finished sample
        self.event: Optional[torch.cuda.Event] = None
        last = walk[-1][3]
        # what _forward_denoising returns: the state turned one-hot (a walk that stops above t = 1, or a vote that keeps x_t), the
        # posterior ("confidence"), or the one-hot of its argmax ("majority")
        self.kind = "state" if last in (hip.STEP_SAMPLE, hip.STEP_LAST_KEEP) else "probs" if last == hip.STEP_LAST_CONFIDENCE else "onehot"

    @property
    def done(self) -> bool:
        return self.finished == self.n

    def result(self) -> Dict[str, torch.Tensor]:
        if self.dropped:
            raise RuntimeError("this request was dropped by SamplingQueue.reset()")
        q = self.queue
        while not self.done:
            q.step()
        self.event.synchronize()
        if int(self.flag.item()) != 0:
            q._flagged = True
            q._engine.raise_range_error()
        H, W = q.image_shape[1:]
        # the rows are complete (the event): the caller's stream may read them; they were allocated on the engine's
        self.buf.record_stream(torch.cuda.current_stream(self.buf.device))
        if self.kind == "state":
            idx = self.buf.reshape(self.n, H, W).long()
            out = torch.nn.functional.one_hot(idx, q.K).permute(0, 3, 1, 2).to(torch.float32)
        else:
            out = self.buf.permute(0, 3, 1, 2)          # BCHW view of channels-last memory, like the solo call's
        if out.device != self.out_device:
            out = out.to(self.out_device)
        return {"diffusion_out": out}


class SamplingQueue:
    """Continuous batching on one engine of `capacity` rows (module docstring).  image_shape = (C, H, W) of the conditioning image.
    guided: requests take evidence=, known_labels=, temperature= and truncation=, and every tick's step is ccdm_slots_guided_step;
    without it the queue is the plain one, launch for launch.  stats: ticks run, busy and idle slot-steps, requests finished.  Not
    thread-safe."""

    RING = 4          # pinned upload buffers: a tick's rowmap and tables stay untouched until the copy that reads them has run

    def __init__(self, model: DenoisingModel, capacity: int, image_shape: Sequence[int], guided: bool = False):
        self.guided = bool(guided)
        if int(capacity) < 1:
            raise ValueError(f"capacity: {capacity} (at least one slot)")
        if len(tuple(image_shape)) != 3:
            raise ValueError(f"image_shape: {tuple(image_shape)} (expected (C, H, W))")
        self.model, self.capacity = model, int(capacity)
        self.image_shape = tuple(int(v) for v in image_shape)
        self.K = int(model.diffusion.num_classes)
        self._check_model()
        self._engine = None
        self._engine_key = None
        self._requests: Dict[int, QueueRequest] = {}
        self._next_id = 0
        self._flagged = False
        self._clear()
        self.stats = dict(ticks=0, busy_slot_steps=0, idle_slot_steps=0, requests_finished=0)

    def _clear(self) -> None:
        self._slots: Slots = (None,) * self.capacity
        self._pending: Pending = ()
        for r in self._requests.values():
            r.dropped = True
        self._requests = {}

    # ------------------------------------------------------------------ checks
    def _check_model(self) -> None:
        m = self.model
        if m.training:
            raise ValueError("training: a sampling queue needs the model in eval mode")
        if m.rng != "philox":
            raise ValueError(f"rng = {m.rng!r}: the queue draws with the device Philox stream only (rng = 'torch_cpu' has no per-slot order)")
        spec = m.unet.spec
        if not spec.softmax_output:
            raise ValueError("softmax_output: no — the network's x0 holds logits; the queue's step needs probabilities")
        if spec.feature_condition_idx:
            raise ValueError("feature_condition: a model that takes one is not built for the queue")

    # ------------------------------------------------------------------ engine
    def _settings_key(self):
        m = self.model
        return (m._weights_key(), m.prec, frozenset(m.f32_layers), m.slicing)

    def _get_engine(self):
        """The queue's own engine for the model's current weights and arithmetic (rebuilt when they change, which needs an empty
        queue: the slots' states live in the engine)."""
        key = self._settings_key()
        if self._engine is not None and key == self._engine_key:
            return self._engine
        if self._requests:
            raise RuntimeError("the model's weights, prec, f32_layers or slicing changed while requests are in flight: reset() the queue")
        m, (Ci, H, W), N, K = self.model, self.image_shape, self.capacity, self.K
        x = torch.empty((N, K, H, W), device="meta")
        cond = torch.empty((N, Ci, H, W), device="meta")
        slot = ("queue", id(self))
        eng = m._engine(x, cond, None, slot=slot)
        # the queue owns this engine: no plain call and no other queue shares it, and the model's cache does not keep it alive
        m._engines = {k: v for k, v in m._engines.items() if k[7] != slot}
        T = m.time_steps
        dev = eng.device
        with eng.enter():
            # every slot holds a valid state from the start: class 0 and a zero image — an idle slot's network pass stays finite
            self._idle_xt = torch.zeros((N, H, W), dtype=torch.uint8, device=dev)
            self._idle_cond = torch.zeros((N, Ci, H, W), dtype=torch.float32, device=dev)
            eng.set_slot_inputs(0, self._idle_xt, self._idle_cond)
            # all T levels, row T - t holds timestep t; every row's network pass stops at x0
            ts = list(range(T, 0, -1))
            eng.set_tables([float(t) for t in ts], [(*m.diffusion.posterior_coeffs(t), hip.STEP_SOFTMAX_ONLY) for t in ts])
            self._table_dev = torch.zeros((N, SLOT_DTYPE.itemsize // 4), dtype=torch.int32, device=dev)
            self._guide_dev = torch.zeros((N, GUIDE_DTYPE.itemsize // 4), dtype=torch.int32, device=dev) if self.guided else None
        eng.leave()
        self._ring = []
        for _ in range(self.RING):
            rows = torch.zeros((N,), dtype=torch.int32).pin_memory()
            tab = torch.zeros((N, SLOT_DTYPE.itemsize // 4), dtype=torch.int32).pin_memory()
            guide = torch.zeros((N, GUIDE_DTYPE.itemsize // 4), dtype=torch.int32).pin_memory() if self.guided else None
            self._ring.append((rows, tab, rows.numpy(), tab.numpy().reshape(-1).view(SLOT_DTYPE), torch.cuda.Event(), guide,
                               None if guide is None else guide.numpy().reshape(-1).view(GUIDE_DTYPE)))
        self._ring_at = 0
        self._engine, self._engine_key = eng, key
        return eng

    @property
    def engine(self):
        """The queue's engine (built on first use)."""
        return self._get_engine()

    # ------------------------------------------------------------------ requests
    def submit(self, condition: torch.Tensor, x: Optional[torch.Tensor] = None, t=None, vote: Optional[str] = None, **guidance) -> QueueRequest:
        """Queue n samples: condition [n,C,H,W]; x the one-hot x_T [n,K,H,W], or None to draw it as predict_single does; t as
        model(x, condition, t=t) takes it (None, an int or a tensor; > 10000 = a strided walk); vote: the last row's vote, default
        model.step_T_sample.  The request takes the Philox key of the model's current `philox_call` and advances it as a call does.
        A guided queue: evidence [n,K,H,W], known_labels [n,H,W], temperature, truncation — meaning, dtypes and errors as
        model(x, condition, ...) has them (the model's own checks)."""
        for k in guidance:
            G.known_keywords("submit", (k,))
            if self.guided and k in QUEUED_GUIDANCE:
                continue
            if self.guided and k in NOT_QUEUED:
                raise ValueError(f"{k}: not built for queued requests ({NOT_QUEUED[k]})")
            raise ValueError(f"{k}: guidance keywords are not built for queued requests")
        self._check_model()
        if self._flagged:
            self._engine.raise_range_error()
        m = self.model
        if condition.dim() != 4 or tuple(condition.shape[1:]) != self.image_shape or condition.shape[0] < 1:
            raise ValueError(f"condition: shape {tuple(condition.shape)}, the queue was built for [n,{','.join(map(str, self.image_shape))}]")
        n, (Ci, H, W) = int(condition.shape[0]), self.image_shape
        if x is not None and tuple(x.shape) != (n, self.K, H, W):
            raise ValueError(f"x: shape {tuple(x.shape)}, expected {(n, self.K, H, W)}")
        init_t = None if t is None else int(t.item()) if isinstance(t, torch.Tensor) else int(t)
        vote = m.step_T_sample if vote is None else vote
        walk = plan_walk(m.time_steps, init_t, vote, m.diffusion.posterior_coeffs)
        # the checks of a solo call, in its order (guidance.check_guidance), before anything is built or counted
        guide = G.check_guidance(m, guidance, (n, self.K, H, W))
        shaping, ev, known = guide.shaping, guide.evidence, guide.known
        eng = self._get_engine()
        if x is None:
            x = OneHotCategoricalBCHW(logits=torch.zeros((n, self.K, H, W), device=condition.device)).sample()
        r = QueueRequest(self, self._next_id, n, int(m.philox_call), m._philox_key(), int(m.sample_offset), vote, walk, init_t, x.device)
        self._next_id += 1
        if shaping is not None or ev is not None or known is not None:
            r.guide = (*(shaping or (1.0, 1.0)), ev is not None, None if known is None else plan_clamp(walk, self.K))
        if m.philox_advance:
            m.philox_call += 1
        dev = eng.device
        with eng.enter():
            # fresh copies made on the engine's stream: the caller's tensors may go away at once
            r.xt_idx = m._to_index(x.to(dev), dev)
            r.cond = condition.to(dev, torch.float32).contiguous().clone()
            r.ev = None if ev is None else ev.to(dev).clone()
            r.known = None if known is None else known.to(dev).clone()
            if r.kind == "state":
                r.buf = torch.empty((n, H * W), dtype=torch.uint8, device=dev)
            else:
                r.buf = torch.empty((n, H, W, self.K), dtype=torch.float32 if r.kind == "probs" else torch.int64, device=dev)
            r.flag = torch.zeros((1,), dtype=torch.int32, device=dev)
        eng.leave()
        r.event = torch.cuda.Event()
        self._requests[r.id] = r
        self._pending = self._pending + tuple((r.id, j) for j in range(n))
        return r

    # ------------------------------------------------------------------ ticks
    @property
    def idle(self) -> bool:
        return not self._pending and all(h is None for h in self._slots)

    def step(self, ticks: int = 1) -> None:
        """Run `ticks` ticks (asynchronous on the engine's stream; a tick with nothing held or waiting is not run)."""
        for _ in range(int(ticks)):
            if self.idle:
                return
            self._tick()

    def run_until_idle(self) -> None:
        while not self.idle:
            self._tick()

    def _tick(self) -> None:
        if self._flagged:
            self._engine.raise_range_error()
        eng = self._get_engine()
        reqs = self._requests
        self._slots, self._pending, admitted, active, finished = schedule_tick(self._slots, self._pending, {i: len(r.walk) for i, r in reqs.items()})
        rows_pin, tab_pin, rows_np, tab_np, ev, guide_pin, guide_np = self._ring[self._ring_at]
        self._ring_at = (self._ring_at + 1) % self.RING
        ev.synchronize()                          # the copies that read these buffers RING ticks ago have run (never recorded: returns at once)
        slot_rows(self.capacity, active, {i: r.walk for i, r in reqs.items()}, {i: r.key for i, r in reqs.items()},
                  {i: r.sample0 for i, r in reqs.items()}, rows_np, tab_np)
        if self.guided:
            slot_guide_rows(self.capacity, active, {i: r.guide for i, r in reqs.items() if r.guide is not None}, guide_np)
        with eng.enter():
            # 1. admissions: runs of consecutive slots that take consecutive samples of one request go in one call
            g = 0
            while g < len(admitted):
                s0, rid, j0 = admitted[g]
                e = g + 1
                while e < len(admitted) and admitted[e] == (s0 + e - g, rid, j0 + e - g):
                    e += 1
                r = reqs[rid]
                eng.set_slot_inputs(s0, r.xt_idx[j0:j0 + e - g], r.cond[j0:j0 + e - g])
                if r.ev is not None or r.known is not None:
                    eng.set_slot_guidance(s0, None if r.ev is None else r.ev[j0:j0 + e - g], None if r.known is None else r.known[j0:j0 + e - g])
                g = e
            # 2. this tick's rowmap and slot table (a guided queue: and its guide table)
            eng.set_rows(rows_pin, non_blocking=True)
            self._table_dev.copy_(tab_pin, non_blocking=True)
            if self.guided:
                self._guide_dev.copy_(guide_pin, non_blocking=True)
            ev.record(eng.stream)
            # 3. the network pass to x0, 4. every slot's own reverse step
            eng.run(1, first_row=0, use_graph=bool(self.model.use_graph))
            if self.guided:
                eng.slots_guided_step(self._table_dev, self._guide_dev)
            else:
                eng.slots_step(self._table_dev)
            # 5. results of the walks that ended
            for s, rid, j in finished:
                r = reqs[rid]
                src = eng.xt if r.kind == "state" else eng.out_probs if r.kind == "probs" else eng.out_onehot
                r.buf[j].copy_(src[s])
                r.flag.copy_(eng.flag)
                r.event.record(eng.stream)
                r.finished += 1
                if r.done:
                    r.cond = r.xt_idx = r.ev = r.known = None         # (allocated on the engine's stream: their memory is reused in stream order)
                    del reqs[rid]
                    self.stats["requests_finished"] += 1
        eng.leave()
        self.stats["ticks"] += 1
        self.stats["busy_slot_steps"] += len(active)
        self.stats["idle_slot_steps"] += self.capacity - len(active)

    def reset(self) -> None:
        """Clear the engine's range flag and drop everything in flight or waiting (their result() raises); every slot goes back to
        the idle state.  The queue is usable again."""
        self._clear()
        self._flagged = False
        if self._engine is not None:
            eng = self._engine
            with eng.enter():
                eng.flag.zero_()
                eng.set_slot_inputs(0, self._idle_xt, self._idle_cond)
            eng.leave()
