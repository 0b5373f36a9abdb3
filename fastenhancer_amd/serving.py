"""StreamPool: streams that join and leave one state buffer (fe_step_slots / fe_state_reset_slots; BSRNN, FSPEN, LiSenNet: fe_step_pool).

The pool owns a state buffer sized for `capacity` streams.  open() hands out a free slot and resets its state; close() frees it;
step() advances only the streams named, each reading and writing its own slot - no gather or scatter of state; step_host() does the
same for audio in page-locked host memory (fe_step_slots_pinned).  No threads, no queues: the caller decides which streams have a hop
ready on each tick.

PacketPool: a StreamPool for PACKET audio - int16 PCM that arrives in pieces of any length (10 or 20 ms packets against a hop of 256
samples, with network jitter).  push() copies a packet into the stream's page-locked ring, tick() is ONE fe_step_streams_pinned launch in
which every stream advances by the whole hops it has, pull() returns the enhanced PCM.  The kernel reads and writes the rings themselves.
set_suppression_limit() bounds how far a stream may be attenuated and levels() reads the stream's input / output level meters: both run
inside the same launch (fe_step_streams_ctl_pinned).  open(bank=) / set_bank() put a stream on another of the engine's weight banks - another
checkpoint of the same shape - still in that one launch (fe_step_streams_banked_pinned).

Moving a stream: export() gathers the state records of open slots (fe_state_export_slots: a record is the stream's state as a capacity-1
state buffer), adopt() opens slots for records made elsewhere, move() takes a live stream to another pool - of another engine of the same
config, on another GPU if need be - and resize() grows or shrinks a pool in place.  PacketPool carries the stream's rings along.

ResampledPacketPool: a PacketPool behind two polyphase resamplers (fastenhancer_amd.resample) for clients at another sample rate - a
telephone leg at 8 kHz, a WebRTC leg at 48 kHz: push() and pull() speak the client's rate, the model runs at its own.  It uses the inner
pool's public methods only: model-rate audio passes through two staging buffers on the host, and a tick waits three times.

RingResampledPacketPool: the same surface and, call for call, the same samples, with the two resamplers reading and writing the inner
pool's rings themselves (Resampler.step_rings_pinned: descriptors that address a ring, with wrap-around).  tick() chains the launch to the
model's rate, the inner pool's launches (PacketPool._enqueue) and the launch back to the client's rate on one stream and waits once; no
model-rate audio is copied on the host.  Any PacketPool class may be the inner pool (pool=FamilyPacketPool, BacklogPacketPool).  What
remains for later: the filter fused into the frame kernels' own sample reads and row stores."""
from __future__ import annotations

import math
import operator
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import torch
from torch import Tensor

from . import _lib
from .engine import Engine
from .family import chunk_step, packet_chunk_on_request, packet_chunk_step, packet_ctl_step, packet_step, pool_family_name, slot_step
from .resample import Resampler


class StreamPool:
    def __init__(self, engine: Engine, capacity: int):
        if capacity < 1:
            raise ValueError("capacity must be at least 1")
        self.engine = engine
        self.capacity = int(capacity)
        self.state = self._new_state(self.capacity)
        self._free: List[int] = list(range(self.capacity - 1, -1, -1))      # popped from the end: lowest slot first
        self._open = set()

    def _new_state(self, capacity: int) -> Tensor:
        """engine.new_state; for a family that steps through fe_step_pool also fe_state_init, which sizes the scratch that step runs on (it
        allocates nothing itself: BSRNN's three-launch step needs its scratch sized for the pool's capacity beforehand)"""
        state = self.engine.new_state(capacity)
        fam = getattr(self.engine, "family", None)
        return self.engine.init_state(state, capacity) if fam is not None and getattr(fam, "pool", False) and state.is_cuda else state

    @property
    def active(self) -> List[int]:
        return sorted(self._open)

    def open(self) -> int:
        """A free slot, its state reset (what a fresh fe_state_init leaves)."""
        if not self._free:
            raise RuntimeError(f"all {self.capacity} slots are open")
        slot = self._free.pop()
        fam = getattr(self.engine, "family", None)
        if fam is not None and fam.arch != _lib.FE_ARCH_FASTENHANCER:
            # BSRNN, FSPEN, LiSenNet: fe_state_reset_slots is built for the FastEnhancer family; their fresh state is zeros, and the state
            # records are built for every family - the slot takes a zero record (such a pool steps through fe_step_pool, a PacketPool
            # through fe_step_pool_streams_pinned; step_host stays FastEnhancer's)
            fresh = torch.zeros(1, self.engine.record_floats, dtype=torch.float32, device=self.state.device)
            self.engine.import_slots(self.state, self.capacity, [slot], fresh)
        else:
            self.engine.reset_slots(self.state, self.capacity, [slot])
        self._open.add(slot)
        return slot

    def close(self, slot: int) -> None:
        if slot not in self._open:
            raise ValueError(f"slot {slot} is not open")
        self._open.remove(slot)
        self._free.append(slot)

    def step(self, slots: Sequence[int], wav_in: Tensor, wav_out: Optional[Tensor] = None, T: int = 1) -> Tensor:
        """wav_in [n, T*H] (row i: stream slots[i]) -> wav_out [n, T*H]; the other streams' state is untouched.  (Engine.step_slots; a
        BSRNN, FSPEN or LiSenNet engine: Engine.step_pool.)"""
        for s in slots:
            if s not in self._open:
                raise ValueError(f"slot {s} is not open")
        return slot_step(self.engine)(wav_in, self.state, self.capacity, list(slots), wav_out=wav_out, T=T)

    def step_host(self, slots: Sequence[int], wav_in: Tensor, wav_out: Optional[Tensor] = None, T: int = 1) -> Tensor:
        """step() for audio in page-locked HOST memory (fe_step_slots_pinned): wav_in [n, T*H] pinned -> wav_out [n, T*H] pinned
        (allocated when None), in one launch.  Asynchronous on the current stream: synchronise it before reading wav_out."""
        for s in slots:
            if s not in self._open:
                raise ValueError(f"slot {s} is not open")
        return self.engine.step_slots_pinned(wav_in, self.state, self.capacity, list(slots), wav_out=wav_out, T=T)

    def catch_up(self, slot: int, wav_in: Tensor, T: Optional[int] = None) -> Tensor:
        """A live stream that comes back with a backlog: wav_in [T*H] or [1, T*H] (T defaults to its length // H) -> the T*H output samples
        [1, T*H], the slot's state advanced by T hops - on the time pipeline (Engine.step_chunk; BSRNN and FSPEN: Engine.step_backlog; LiSenNet: after
        Engine.set_time_pipeline(P >= 2), else the walk) instead of hop after hop.  The slot's state record is a capacity-1 state: it is exported, stepped as a batch of one, and imported back; no other slot is read or written.
        The result agrees with step() over the same hops to fp32 rounding."""
        if slot not in self._open:
            raise ValueError(f"slot {slot} is not open")
        if wav_in.dim() == 1:
            wav_in = wav_in.unsqueeze(0)
        if wav_in.dim() != 2 or wav_in.shape[0] != 1:
            raise ValueError("catch_up takes the backlog of ONE stream: wav_in [T*H] or [1, T*H]")
        rec = self.engine.export_slots(self.state, self.capacity, [slot])
        out = chunk_step(self.engine)(wav_in, rec.view(-1), T=T)
        self.engine.import_slots(self.state, self.capacity, [slot], rec)
        return out

    # ---- moving live streams (fe_state_export_slots / fe_state_import_slots)
    def export(self, slots: Sequence[int], pinned: bool = False) -> Tensor:
        """The state records [n, record_floats] of the named open slots, on the engine's device or (pinned) in page-locked host memory - then
        synchronise the engine before reading them.  The slots stay open: close() drops them."""
        slots = list(slots)
        for s in slots:
            if s not in self._open:
                raise ValueError(f"slot {s} is not open")
        out = self.engine.new_pinned(len(slots), self.engine.record_floats) if pinned else None
        return self.engine.export_slots(self.state, self.capacity, slots, out=out)

    def adopt(self, records: Tensor) -> List[int]:
        """Opens one free slot per record [n, record_floats] and imports the record into it (no reset first); the slots in record order.
        Raises when there are not enough free slots, and opens none then."""
        n = int(records.shape[0])
        if n > len(self._free):
            raise RuntimeError(f"{n} records for {len(self._free)} free slots of {self.capacity}")
        if n == 0:
            return []
        slots = self._free[-n:][::-1]                     # (what n pops would hand out; taken off the list once the import is enqueued)
        self.engine.import_slots(self.state, self.capacity, slots, records)
        del self._free[-n:]
        self._open.update(slots)
        return slots

    def _check_move(self, slot: int, dst_pool: "StreamPool") -> None:
        """what move() refuses before anything is copied"""
        if slot not in self._open:
            raise ValueError(f"slot {slot} is not open")
        a, b = getattr(self.engine, "cfg", None), getattr(dst_pool.engine, "cfg", None)
        if type(a) is not type(b) or a != b:
            raise ValueError("the pools' engines have different configs: a state record is valid for one config only")
        if not dst_pool._free:
            raise RuntimeError(f"all {dst_pool.capacity} slots of the destination are open")

    def move(self, slot: int, dst_pool: "StreamPool") -> int:
        """Takes the live stream in `slot` to dst_pool (export, adopt there, close here) and returns its slot there.  The pools may belong
        to different engines of the same config, on different devices: the record then travels through page-locked host memory (export to
        it, synchronise, import from it on the other device), which needs no peer access."""
        self._check_move(slot, dst_pool)
        same = getattr(self.engine, "device", None) == getattr(dst_pool.engine, "device", None)
        rec = self.export([slot], pinned=not same)
        if not same:
            self.engine.synchronize()
        new = dst_pool.adopt(rec)[0]
        if not same:
            dst_pool.engine.synchronize()                 # (the host record is released when this returns)
        self.close(slot)
        return new

    def resize(self, capacity: int) -> None:
        """Grows or shrinks the pool to `capacity` slots: a new state buffer (engine.new_state), every open stream exported and imported at
        the SAME slot number, the free list rebuilt.  Shrinking below 1 + the highest open slot raises and changes nothing.  The old state
        tensor is not reused: a caller that holds pool.state must read it again."""
        capacity = int(capacity)
        if capacity < 1:
            raise ValueError("capacity must be at least 1")
        if self._open and capacity < 1 + max(self._open):
            raise ValueError(f"slot {max(self._open)} is open: the pool cannot shrink below {1 + max(self._open)} slots")
        if capacity == self.capacity:
            return
        state = self._new_state(capacity)
        if self._open:
            slots = sorted(self._open)
            self.engine.import_slots(state, capacity, slots, self.engine.export_slots(self.state, self.capacity, slots))
        self.state = state
        self.capacity = capacity
        self._free = [s for s in range(capacity - 1, -1, -1) if s not in self._open]


def carry_ring(src_in: Tensor, src_out: Tensor, pushed: int, stepped: int, pulled: int, dst_in: Tensor, dst_out: Tensor) -> Tuple[int, int, int]:
    """What a packet stream has in flight, from one slot's rings (1-D, src_in / src_out) to another's (dst_in / dst_out, of any other
    length): input samples stepped <= k < pushed (pushed, not yet stepped) and output samples pulled <= k < stepped (stepped, not yet
    pulled).  The stream's sample k sits at position k mod ring on both sides, so the sample numbering - the three counters, which are
    returned - carries over as it is and the next push / tick / pull find everything in place.  OverflowError, before anything is copied,
    if pushed - pulled exceeds the destination ring."""
    rs, rd = src_in.numel(), dst_in.numel()
    if src_out.numel() != rs or dst_out.numel() != rd:
        raise ValueError("the input and output ring of a slot have one length")
    if not 0 <= pulled <= stepped <= pushed or pushed - pulled > rs:
        raise ValueError(f"counters pulled {pulled} <= stepped {stepped} <= pushed {pushed} do not describe a ring of {rs} samples")
    if pushed - pulled > rd:
        raise OverflowError(f"{pushed - pulled} samples in flight do not fit the destination ring of {rd} samples")
    k = torch.arange(stepped, pushed, dtype=torch.int64)
    dst_in[k % rd] = src_in[k % rs]
    k = torch.arange(pulled, stepped, dtype=torch.int64)
    dst_out[k % rd] = src_out[k % rs]
    return pushed, stepped, pulled


def _dbfs(amplitude: float) -> float:
    return 20.0 * math.log10(amplitude) if amplitude > 0.0 else -math.inf


@dataclass(frozen=True)
class StreamLevels:
    """What the kernel metered for one stream on its last tick with a hop: sum of squares and peak of the `samples` input samples it read
    and of the output samples it wrote (floats, full scale 1.0; the output before its int16 quantisation).  samples = 0: nothing yet."""
    in_sumsq: float = 0.0
    in_peak: float = 0.0
    out_sumsq: float = 0.0
    out_peak: float = 0.0
    samples: int = 0

    @property
    def in_rms_dbfs(self) -> float:
        return _dbfs(math.sqrt(self.in_sumsq / self.samples)) if self.samples else -math.inf

    @property
    def out_rms_dbfs(self) -> float:
        return _dbfs(math.sqrt(self.out_sumsq / self.samples)) if self.samples else -math.inf

    @property
    def in_peak_dbfs(self) -> float:
        return _dbfs(self.in_peak)

    @property
    def out_peak_dbfs(self) -> float:
        return _dbfs(self.out_peak)


class PacketPool(StreamPool):
    """Streams fed by int16 PCM packets of any length.  Every slot has an input and an output ring of ring_hops * H samples in page-locked
    host memory; a stream's sample k lives at ring position k mod (ring_hops * H) of both.  Between the oldest sample not yet pulled and
    the newest one pushed a stream may hold one ring of samples: push() refuses what would overwrite them.  No threads, no queues.
    meters=True: every tick also meters each launched stream's input and output (levels()).  The level table lives in page-locked host
    memory - tick() synchronises anyway - and the table of suppression limits, made by the first set_suppression_limit(), on the device;
    a pool with neither launches plain fe_step_streams_pinned.  The table of weight banks, made by the first open(bank=) / set_bank() that
    names a bank other than 0, lives on the device too; a pool that never names one launches what it launched without banks.
    backlog_hops = K >= 4: a stream that holds more than T_max complete hops (up to its ring end) - one that comes back after a stall -
    is taken out of the tick's ordinary launch and served, up to K hops a tick, by a second launch on the time pipeline
    (Engine.step_streams_chunk_pinned: same slot, bank, limit and meters), so the other streams' launch stays T_max hops long.  0 (the
    default): one launch, as ever.
    A BSRNN, FSPEN or LiSenNet engine: tick() launches Engine.step_pool_streams_pinned (fe_step_pool_streams_pinned); push, pull, move,
    resize, adopt, export and catch_up work as for FastEnhancer.  The meters, the suppression limit, the weight banks and backlog_hops are
    FastEnhancer's: such a pool refuses them with a ValueError that names the family, before it calls the engine.  (FamilyPacketPool, below,
    has the meters and the limit for those families too, BacklogPacketPool backlog_hops as well.)"""

    def __init__(self, engine: Engine, capacity: int, ring_hops: int, T_max: int = 1, meters: bool = False, backlog_hops: int = 0):
        self._baseline = pool_family_name(engine)          # "BSRNN" / "FSPEN" / "LiSenNet", or None: the per-stream controls are available
        if meters:
            self._refuse_baseline("level meters (meters=True)")
        if backlog_hops != 0:
            self._refuse_baseline("the pipelined packet step (backlog_hops)")
        super().__init__(engine, capacity)
        if ring_hops < 1 or T_max < 1:
            raise ValueError("ring_hops and T_max must be at least 1")
        backlog_hops = operator.index(backlog_hops)
        if backlog_hops != 0 and (backlog_hops < 4 or backlog_hops <= T_max):
            raise ValueError("backlog_hops is 0 (off) or at least 4 hops (what the time pipeline takes) and more than T_max")
        self.backlog_hops = backlog_hops
        self._backlog_work: Optional[Tensor] = None        # the chunk launch's scratch, made once for (capacity, backlog_hops)
        self._gain: Optional[Tensor] = None                # [capacity] linear least gain per slot, 0 = off
        self._bank: Optional[Tensor] = None                # [capacity] int32 weight bank per slot (None: every stream on bank 0)
        self._levels: Optional[Tensor] = engine.new_pinned(self.capacity, 4) if meters else None
        self._level_samples = [0] * self.capacity          # samples behind each level row (0: no row yet)
        self.H = int(engine.cfg.hop_size)
        self.ring = int(ring_hops) * self.H
        self.T_max = int(T_max)
        self.ring_in = engine.new_pinned(self.capacity, self.ring, dtype=torch.int16)
        self.ring_out = engine.new_pinned(self.capacity, self.ring, dtype=torch.int16)
        # per slot, in samples since open(): pushed >= stepped (a multiple of H) >= pulled
        self._pushed = [0] * self.capacity
        self._stepped = [0] * self.capacity
        self._pulled = [0] * self.capacity

    def _refuse_baseline(self, what: str) -> None:
        if self._baseline is not None:
            raise ValueError(f"a PacketPool of a {self._baseline} engine has no {what}: suppression limits, level meters, weight banks and the "
                             "pipelined packet step are built for the FastEnhancer family")

    def _reset_ctl(self, slot: int) -> None:
        """limit off, no level row"""
        if self._gain is not None:
            self._gain[slot] = 0.0
        if self._levels is not None:
            self._levels[slot] = 0.0
        self._level_samples[slot] = 0

    def open(self, bank: int = 0) -> int:
        """StreamPool.open; the stream runs on weight bank `bank` of the engine (ValueError, and no slot is opened, outside its banks)."""
        if bank != 0:
            self._refuse_baseline(f"weight bank {bank!r}")
        bank = self._check_bank(bank, self.engine)
        slot = super().open()
        self._pushed[slot] = self._stepped[slot] = self._pulled[slot] = 0
        self._reset_ctl(slot)
        self._set_bank(slot, bank)
        return slot

    def adopt(self, records: Tensor) -> List[int]:
        """StreamPool.adopt; the adopted streams start with empty rings, no limit and no level row, on bank 0 (move() carries a stream's
        rings, limit and bank along)."""
        slots = super().adopt(records)
        for slot in slots:
            self._pushed[slot] = self._stepped[slot] = self._pulled[slot] = 0
            self._reset_ctl(slot)
            self._set_bank(slot, 0)
        return slots

    def catch_up(self, slot: int, wav_in: Tensor, T: Optional[int] = None) -> Tensor:
        """StreamPool.catch_up for a stream on bank 0 without a suppression limit (it takes float audio past the rings, leaves the
        counters and the level row alone, and runs on bank 0 without a limit: Engine.step_chunk knows neither).  A stream on another bank or
        with a limit is refused - its audio would be enhanced by another checkpoint, or unlimited: serve its backlog through the rings with
        PacketPool(..., backlog_hops=K)."""
        self._check_open(slot)
        if self._bank is not None and int(self._bank[slot]) != 0:
            raise ValueError(f"slot {slot} runs on weight bank {int(self._bank[slot])} and catch_up on bank 0: push the backlog and let tick() serve it "
                             "(PacketPool(..., backlog_hops=K))")
        if self._get_gain(slot) != 0.0:
            raise ValueError(f"slot {slot} has a suppression limit, which catch_up does not apply: push the backlog and let tick() serve it "
                             "(PacketPool(..., backlog_hops=K))")
        return super().catch_up(slot, wav_in, T)

    # ---- weight banks: streams of one pool on different checkpoints (fe_step_streams_banked_pinned)
    @staticmethod
    def _check_bank(bank, engine) -> int:
        n = int(getattr(engine, "weight_banks", 1))
        try:
            k = -1 if isinstance(bank, bool) else operator.index(bank)
        except TypeError:
            k = -1
        if not 0 <= k < n:
            raise ValueError(f"bank {bank!r} is outside the engine's banks [0, {n})")
        return k

    def _set_bank(self, slot: int, bank: int) -> None:
        if self._bank is None:
            if bank == 0:
                return
            self._bank = torch.zeros(self.capacity, dtype=torch.int32, device=getattr(self.engine, "device", None))
        self._bank[slot] = bank

    def set_bank(self, slot: int, bank: int) -> None:
        """The stream runs on weight bank `bank` from the next tick on.  (Its state carries over - the layout is the same - but what a
        stream sounds like across a change of checkpoint is the checkpoints' business.)"""
        self._check_open(slot)
        if bank != 0:
            self._refuse_baseline(f"weight bank {bank!r}")
        self._set_bank(slot, self._check_bank(bank, self.engine))

    def bank(self, slot: int) -> int:
        """the weight bank the stream runs on"""
        self._check_open(slot)
        return 0 if self._bank is None else int(self._bank[slot])

    # ---- the suppression limit and the level meters (fe_step_streams_ctl_pinned)
    @staticmethod
    def _limit_gain(db: Optional[float]) -> float:
        """dB (<= 0; None or -inf: off) -> the linear least gain of the kernel's table (0 = off)"""
        if db is None:
            return 0.0
        db = float(db)
        if math.isnan(db) or db > 0.0:
            raise ValueError(f"a suppression limit is a level in dB at or below 0 (None or -inf: no limit), got {db}")
        return 0.0 if math.isinf(db) else 10.0 ** (db / 20.0)

    def set_suppression_limit(self, slot: int, db: Optional[float]) -> None:
        """No bin of the stream is attenuated by more than `db` (-20.0: at most 20 dB of suppression) from the next tick on; None or -inf
        lifts the limit.  Open streams start without one."""
        self._check_open(slot)
        gain = self._limit_gain(db)
        if gain != 0.0:
            self._refuse_baseline("suppression limit")
        self._set_gain(slot, gain)

    def _get_gain(self, slot: int) -> float:
        return 0.0 if self._gain is None else float(self._gain[slot])

    def _set_gain(self, slot: int, gain: float) -> None:
        if self._gain is None:
            if gain == 0.0:
                return
            self._gain = torch.zeros(self.capacity, dtype=torch.float32, device=getattr(self.engine, "device", None))
        self._gain[slot] = gain

    def suppression_limit(self, slot: int) -> Optional[float]:
        """the stream's limit in dB, None when it has none"""
        self._check_open(slot)
        gain = self._get_gain(slot)
        return 20.0 * math.log10(gain) if gain > 0.0 else None

    def levels(self, slot: int) -> StreamLevels:
        """The level row of the stream's last tick with at least one hop (StreamLevels; samples = 0 before the first)."""
        self._check_open(slot)
        if self._levels is None:
            raise RuntimeError("the pool was made without meters (PacketPool(..., meters=True))")
        if not self._level_samples[slot]:
            return StreamLevels()
        return StreamLevels(*(float(v) for v in self._levels[slot]), samples=self._level_samples[slot])

    def move(self, slot: int, dst_pool: "PacketPool") -> int:
        """StreamPool.move with the packet side: what the stream has in flight - samples pushed but not yet stepped, samples stepped but
        not yet pulled - and its three counters go to dst_pool's rings (carry_ring), which may have another ring_hops.  OverflowError,
        before anything is copied, if that does not fit the destination ring.  The stream's next push / tick / pull on dst_pool behave as
        if it had always lived there."""
        if not isinstance(dst_pool, PacketPool):
            raise TypeError("a packet stream moves to a PacketPool")
        self._check_move(slot, dst_pool)
        bank = self._check_bank(self.bank(slot), dst_pool.engine)       # (the destination engine must have the stream's bank)
        counters = (self._pushed[slot], self._stepped[slot], self._pulled[slot])
        if counters[0] - counters[2] > dst_pool.ring:
            raise OverflowError(f"slot {slot}: {counters[0] - counters[2]} samples in flight do not fit the destination ring of {dst_pool.ring} samples")
        src_in, src_out = self.ring_in[slot].clone(), self.ring_out[slot].clone()      # (close() may hand the slot out again)
        gain = self._get_gain(slot)                         # (the table's own float: the limit moves bit for bit)
        new = super().move(slot, dst_pool)
        p = carry_ring(src_in, src_out, *counters, dst_pool.ring_in[new], dst_pool.ring_out[new])
        dst_pool._pushed[new], dst_pool._stepped[new], dst_pool._pulled[new] = p
        dst_pool._set_gain(new, gain)
        dst_pool._set_bank(new, bank)
        return new

    def resize(self, capacity: int) -> None:
        """StreamPool.resize with the packet side: new rings of the same ring_hops, the open slots' rows and counters at the same slot
        numbers.  pool.ring_in / pool.ring_out are new tensors, like pool.state."""
        old = self.capacity
        super().resize(capacity)
        if self.capacity == old:
            return
        self._backlog_work = None                           # (sized for the capacity: made again by the next backlog tick)
        keep = min(old, self.capacity)
        rings = []
        for ring in (self.ring_in, self.ring_out):
            new = self.engine.new_pinned(self.capacity, self.ring, dtype=torch.int16)
            new[:keep] = ring[:keep]
            rings.append(new)
        self.ring_in, self.ring_out = rings
        grow = [0] * (self.capacity - keep)
        self._pushed, self._stepped, self._pulled = (c[:keep] + grow for c in (self._pushed, self._stepped, self._pulled))
        self._level_samples = self._level_samples[:keep] + grow
        if self._gain is not None:
            gain = torch.zeros(self.capacity, dtype=torch.float32, device=self._gain.device)
            gain[:keep] = self._gain[:keep]
            self._gain = gain
        if self._bank is not None:
            bank = torch.zeros(self.capacity, dtype=torch.int32, device=self._bank.device)
            bank[:keep] = self._bank[:keep]
            self._bank = bank
        if self._levels is not None:
            levels = self.engine.new_pinned(self.capacity, 4)
            levels[:keep] = self._levels[:keep]
            self._levels = levels

    def _check_open(self, slot: int) -> None:
        if slot not in self._open:
            raise ValueError(f"slot {slot} is not open")

    def push(self, slot: int, pcm) -> None:
        """Append a packet: a 1-D int16 array or tensor of any length.  The copy wraps at the ring end."""
        self._check_open(slot)
        x = torch.as_tensor(pcm)
        if x.dim() != 1 or x.dtype != torch.int16:
            raise ValueError(f"a packet is a 1-D int16 array, got {x.dtype} {tuple(x.shape)}")
        n = x.numel()
        pos = self._reserve_push(slot, n)
        first = min(n, self.ring - pos)
        self.ring_in[slot, pos:pos + first] = x[:first]
        if first < n:
            self.ring_in[slot, :n - first] = x[first:]

    def _reserve_push(self, slot: int, n: int) -> int:
        """The input ring's bookkeeping for n new samples: OverflowError, and nothing taken, when they would overwrite samples not yet pulled;
        else the slot has pushed n more, and the ring position of the first of them is returned (they wrap at the ring end).  Whoever calls
        this writes the samples there before the next tick: push(), or a launch that writes into the ring (RingResampledPacketPool)."""
        w = self._pushed[slot]
        if w + n - self._pulled[slot] > self.ring:
            raise OverflowError(f"slot {slot}: {n} samples do not fit - the ring holds {self.ring} samples between pull() and push(), "
                                f"{w - self._pulled[slot]} are in it")
        self._pushed[slot] = w + n
        return w % self.ring

    def _reserve_pull(self, slot: int) -> Tuple[int, int]:
        """The output ring's bookkeeping for everything stepped since the last pull: (ring position of the first sample, count) - they wrap at
        the ring end - and the slot has pulled them."""
        r, n = self._pulled[slot], self._stepped[slot] - self._pulled[slot]
        self._pulled[slot] = r + n
        return r % self.ring, n

    def tick(self) -> List[Tuple[int, int, int, int]]:
        """One launch (Engine.step_streams_pinned; a BSRNN, FSPEN or LiSenNet engine: Engine.step_pool_streams_pinned) for every open stream
        with at least one complete hop: each advances min(complete hops, hops up to the ring end, T_max); the rest waits for the next tick.  With backlog_hops = K, a stream whose complete hops up to the ring end exceed T_max
        advances min(complete hops, hops up to the ring end, K) in a second launch on the same stream, on the time pipeline (_backlog_call,
        its scratch sized by _backlog_work_floats: the two hooks BacklogPacketPool answers for the other families).  Waits once,
        for both (the rings are host memory the caller reads next).  Returns the descriptors (slot, hops, in_offset, out_offset) it
        launched, the ordinary launch's first - [] when no stream had a hop, and then nothing is launched.
        (Two parts, _enqueue and _complete, with the wait between them: a pool that chains launches of its own in front of and behind
        these - RingResampledPacketPool - calls the parts and waits once for all of them.)"""
        desc = self._enqueue()
        if desc:
            self.engine.synchronize()
        self._complete(desc)
        return desc

    def _enqueue(self) -> List[Tuple[int, int, int, int]]:
        """tick()'s descriptors and its one or two launches, without the wait; returns the descriptors launched"""
        desc, backlog = [], []
        for slot in sorted(self._open):
            pos = self._stepped[slot] % self.ring
            ready = min((self._pushed[slot] - self._stepped[slot]) // self.H, (self.ring - pos) // self.H)
            off = slot * self.ring + pos
            if self.backlog_hops and ready > self.T_max:
                backlog.append((slot, min(ready, self.backlog_hops), off, off))
            elif ready > 0:
                desc.append((slot, min(ready, self.T_max), off, off))
        if not desc and not backlog:
            return desc
        ctl = {} if self._gain is None and self._levels is None else dict(min_gain=self._gain, levels=self._levels)
        if self._bank is not None:
            ctl["bank"] = self._bank
        if desc:
            self._packet_call(ctl)(self.ring_in, self.state, self.capacity, desc, self.ring_out, T_max=self.T_max, **ctl)
        if backlog:
            if self._backlog_work is None:
                need = self._backlog_work_floats()(self.capacity, self.backlog_hops)
                self._backlog_work = torch.empty(max(need, 1), dtype=torch.float32, device=getattr(self.engine, "device", None))
            self._backlog_call()(self.ring_in, self.state, self.capacity, backlog, self.ring_out, T_max=self.backlog_hops,
                                 min_gain=self._gain, levels=self._levels, bank=self._bank, work=self._backlog_work)
            desc = desc + backlog
        return desc

    def _complete(self, desc) -> None:
        """the counters follow what _enqueue launched, once the stream has been waited for"""
        for slot, hops, _, _ in desc:
            self._stepped[slot] += hops * self.H
            self._level_samples[slot] = hops * self.H

    def _packet_call(self, ctl: dict):
        """the engine's call for the tick's ordinary launch, given the tables it will be handed"""
        return packet_step(self.engine, pinned=True)

    def _backlog_call(self):
        """the engine's call for the tick's backlog launch (min_gain=, levels=, bank=, work=)"""
        return self.engine.step_streams_chunk_pinned

    def _backlog_work_floats(self):
        """... and the query (n, T_max) that sizes its scratch"""
        return self.engine.streams_chunk_work_floats

    def pull(self, slot: int) -> Tensor:
        """The enhanced int16 samples produced since the last pull (a copy; empty when there are none)."""
        self._check_open(slot)
        pos, n = self._reserve_pull(slot)
        first = min(n, self.ring - pos)
        return torch.cat([self.ring_out[slot, pos:pos + first], self.ring_out[slot, :n - first]])


class FamilyPacketPool(PacketPool):
    """A PacketPool whose suppression limit and level meters work for every family.  On a FastEnhancer engine it is PacketPool, call for call.
    On a BSRNN, FSPEN or LiSenNet engine tick() launches Engine.step_pool_streams_pinned while neither control is in use - no meters, no
    limit ever set - and Engine.step_pool_streams_ctl_pinned (fe_step_pool_streams_ctl_pinned) otherwise; set_suppression_limit, levels,
    move, resize and adopt carry the two tables as PacketPool does.  There the limit holds each output bin against the input bin,
    |Y| >= 10^(dB / 20) |X| (the output of these models is not a mask times the input).  Weight banks other than 0 and backlog_hops are
    refused with the family's name (backlog_hops for those families: BacklogPacketPool, below); catch_up keeps refusing a slot with a limit."""

    _FAMILY_CONTROLS = ("level meters", "suppression limit")

    def _refuse_baseline(self, what: str) -> None:
        if self._baseline is not None and not what.startswith(self._FAMILY_CONTROLS):
            raise ValueError(f"a FamilyPacketPool of a {self._baseline} engine has no {what}: weight banks and the pipelined packet step are built "
                             "for the FastEnhancer family")

    def _packet_call(self, ctl: dict):
        if self._baseline is not None and ctl:
            return packet_ctl_step(self.engine, pinned=True)
        return packet_step(self.engine, pinned=True)

    def move(self, slot: int, dst_pool: "PacketPool") -> int:
        """PacketPool.move; a stream with a limit on a BSRNN, FSPEN or LiSenNet engine moves to a FamilyPacketPool only (a plain PacketPool of
        such an engine has no limit to carry it)."""
        if isinstance(dst_pool, PacketPool) and not isinstance(dst_pool, FamilyPacketPool) and dst_pool._baseline is not None \
                and slot in self._open and self._get_gain(slot) != 0.0:
            dst_pool._refuse_baseline("suppression limit")
        return super().move(slot, dst_pool)


class BacklogPacketPool(FamilyPacketPool):
    """A FamilyPacketPool with backlog_hops = K for every family.  On a FastEnhancer engine it is PacketPool, call for call.  On a BSRNN, FSPEN
    or LiSenNet engine a stream with more than T_max complete hops up to the ring end leaves the tick's ordinary launch and advances up to K
    hops in a second launch on the same stream, Engine.step_pool_streams_chunk_pinned (fe_step_pool_streams_chunk_pinned: each stream's hops
    on the time pipeline for BSRNN and FSPEN; for LiSenNet too once the engine's time pipeline was set to an explicit width of two or more,
    Engine.set_time_pipeline(P >= 2), and the packet step itself at every other setting), with its limit and its meters; tick() waits once,
    for both.  Weight banks other than 0 stay FastEnhancer's and are refused with the family's name."""

    _FAMILY_CONTROLS = FamilyPacketPool._FAMILY_CONTROLS + ("the pipelined packet step",)

    def _refuse_baseline(self, what: str) -> None:
        if self._baseline is not None and not what.startswith(self._FAMILY_CONTROLS):
            raise ValueError(f"a BacklogPacketPool of a {self._baseline} engine has no {what}: weight banks are built for the FastEnhancer family")

    def _backlog_call(self):
        if self._baseline is None:
            return super()._backlog_call()
        call = packet_chunk_step(self.engine, pinned=True)
        return lambda *a, bank=None, **kw: call(*a, **kw)       # (no bank table in that call: such a pool has none)

    def _backlog_work_floats(self):
        """The query that sizes the backlog launch's scratch.  A family that pipelines the call on request (LiSenNet) answers with its own
        query when the engine's width is two or more - read when the scratch is first made, so a pool that ticked a backlog before
        Engine.set_time_pipeline(P >= 2) keeps the small scratch (the engine then refuses it by size): resize() makes it again."""
        if self._baseline is None:
            return super()._backlog_work_floats()
        if packet_chunk_on_request(self.engine):
            return self.engine.lisennet_pool_streams_chunk_work_floats
        return self.engine.pool_streams_chunk_work_floats


class ResampledPacketPool:
    """A PacketPool for clients at `client_rate`, the model at `model_rate`.  It holds a PacketPool (`inner`) and two Resamplers with one
    state row per slot each, and uses the inner pool's public methods only, so it serves every family the PacketPool serves.  push() takes
    int16 PCM at the client's rate - up to max_packet samples per slot between two ticks - and pull() returns int16 PCM at the client's rate.
    tick() is five steps in order:
      1. one Resampler.step_streams_pinned launch: every slot's pending input -> model-rate PCM in a page-locked staging buffer;
      2. inner.push of each slot's new model-rate samples;
      3. inner.tick();
      4. inner.pull of every slot;
      5. one Resampler.step_streams_pinned launch back to the client's rate.
    That is three launches and two host hops a tick, where PacketPool has one launch: RingResampledPacketPool, below, resamples straight
    into and out of the inner pool's rings and waits once (this class is its oracle, and the form that needs nothing but the inner pool's
    public methods); fusing the filter into the frame kernels themselves is left for later.  Both resamplers are streaming-exact across packets (the outputs are those of one call on the whole signal),
    each with its own latency of half_len / up input samples; nothing is flushed when a slot closes.
    model_rate: the engine's configuration does not carry a sample rate - 16000 for the 16 kHz configurations, 48000 for the 48 kHz ones.
    client_format: "s16" (the above), or "ulaw" / "alaw" for telephony clients - G.711, one byte per sample (fastenhancer_amd.g711): push()
    then takes a 1-D uint8 array of that law and pull() returns uint8, the client-rate staging buffers are uint8, and the two resampler
    launches decode and encode on their client side (in_format= / out_format=).  The model-rate side, the inner pool and every counter are
    as with "s16": each pull() is the G.711 encoding of what the "s16" pool returns when fed the decoded bytes."""

    def __init__(self, engine: Engine, capacity: int, ring_hops: int, client_rate: int, T_max: int = 1, max_packet: Optional[int] = None, *,
                 model_rate: int = 16000, client_format: str = "s16"):
        self._set_client_format(client_format)
        client_rate, model_rate = operator.index(client_rate), operator.index(model_rate)
        if client_rate == model_rate:
            raise ValueError(f"client_rate {client_rate} is the model's rate: there is nothing to resample, use PacketPool")
        device = getattr(engine, "device", None)
        self.client_rate, self.model_rate = client_rate, model_rate
        self.to_model = self._make_resampler(client_rate, model_rate, device)
        self.to_client = self._make_resampler(model_rate, client_rate, device)
        self.inner = self._make_pool(engine, capacity, ring_hops, T_max)
        self.capacity = int(capacity)
        step = int(self.inner.T_max) * int(self.inner.H)                   # model-rate samples a slot advances per tick at most
        if max_packet is None:                                             # what a tick can take away, at the client's rate
            max_packet = -(-step * client_rate // model_rate)
        self.max_packet = operator.index(max_packet)
        if self.max_packet < 1:
            raise ValueError("max_packet must be at least 1")
        self._model_cap = self.to_model.out_count(self.max_packet) + 1    # model-rate samples of max_packet client samples at most
        self._client_cap = self.to_client.out_count(step) + 1             # client-rate samples of one tick's output at most
        self._step = step
        self.state_in = self.to_model.new_state(self.capacity)
        self.state_out = self.to_client.new_state(self.capacity)
        self._cin = self.to_model.new_pinned(self.capacity, self.max_packet, dtype=self._client_dtype)
        self._min = self.to_model.new_pinned(self.capacity, self._model_cap, dtype=torch.int16)
        self._mout = self.to_client.new_pinned(self.capacity, step, dtype=torch.int16)
        self._cout = self.to_client.new_pinned(self.capacity, self._client_cap, dtype=self._client_dtype)
        self._made_in = self.to_model.new_pinned(self.capacity, dtype=torch.int32)
        self._made_out = self.to_client.new_pinned(self.capacity, dtype=torch.int32)
        self._pending = [0] * self.capacity          # client-rate samples waiting in _cin
        self._consumed = [0] * self.capacity         # client-rate samples the resampler to the model's rate has consumed
        self._fill = [0] * self.capacity             # model-rate samples pushed into the inner pool and not yet pulled from it
        self._ready: List[List[Tensor]] = [[] for _ in range(self.capacity)]
        self._open = set()

    def _set_client_format(self, client_format) -> None:
        """client_format: what push() takes and pull() returns at the client's rate - "s16" (int16 PCM), or "ulaw" / "alaw": G.711, one
        uint8 byte per sample, decoded and encoded by the two resampler launches (Resampler's in_format= / out_format=)"""
        if client_format not in ("s16", "ulaw", "alaw"):
            raise ValueError(f"client_format must be 's16', 'ulaw' or 'alaw', got {client_format!r}")
        self.client_format = client_format
        law = None if client_format == "s16" else client_format
        self._client_dtype = torch.int16 if law is None else torch.uint8
        # the keywords of the two launches' client sides ("s16": none - the calls are what they were)
        self._in_kw = {} if law is None else {"in_format": law}
        self._out_kw = {} if law is None else {"out_format": law}

    # (the two constructors tick() depends on, apart for the tests that record the calls instead of running them)
    @staticmethod
    def _make_pool(engine, capacity, ring_hops, T_max) -> PacketPool:
        return PacketPool(engine, capacity, ring_hops, T_max=T_max)

    @staticmethod
    def _make_resampler(sr_in, sr_out, device) -> Resampler:
        return Resampler(sr_in, sr_out, device)

    @property
    def active(self) -> List[int]:
        return sorted(self._open)

    def _check_open(self, slot: int) -> None:
        if slot not in self._open:
            raise ValueError(f"slot {slot} is not open")

    def _fresh(self, slot: int) -> None:
        self.state_in[slot] = 0.0
        self.state_out[slot] = 0.0
        self._pending[slot] = self._consumed[slot] = self._fill[slot] = 0
        self._ready[slot] = []

    def open(self) -> int:
        """inner.open(); the slot's two resampler rows start as zeros (fresh streams)"""
        slot = self.inner.open()
        self._fresh(slot)
        self._open.add(slot)
        return slot

    def close(self, slot: int) -> None:
        self._check_open(slot)
        self.inner.close(slot)
        self._open.remove(slot)
        self._fresh(slot)

    def push(self, slot: int, pcm) -> None:
        """Append a packet at the client's rate: a 1-D int16 array or tensor.  OverflowError, and nothing taken, when more than max_packet
        samples would wait for the next tick or the inner pool's ring could not hold what they become."""
        self._check_open(slot)
        x = torch.as_tensor(pcm)
        if x.dim() != 1 or x.dtype != self._client_dtype:
            if self.client_format != "s16":
                raise ValueError(f"a packet is a 1-D uint8 array of G.711 {self.client_format} bytes, got {x.dtype} {tuple(x.shape)}")
            raise ValueError(f"a packet is a 1-D int16 array, got {x.dtype} {tuple(x.shape)}")
        n, have = x.numel(), self._pending[slot]
        if have + n > self.max_packet:
            raise OverflowError(f"slot {slot}: {n} samples do not fit - {have} of max_packet = {self.max_packet} samples wait for the next tick")
        if self._fill[slot] + self.to_model.produced(self._consumed[slot], have + n) > self.inner.ring:
            raise OverflowError(f"slot {slot}: {n} samples do not fit - the inner pool's ring holds {self.inner.ring} samples, {self._fill[slot]} are in it")
        self._cin[slot, have:have + n] = x
        self._pending[slot] = have + n

    def tick(self) -> List[Tuple[int, int, int, int]]:
        """The five steps above.  Waits for each of its launches (the staging buffers are host memory it reads next).  Returns what
        inner.tick() returned."""
        todo = [(slot, self._pending[slot], slot * self.max_packet, slot * self._model_cap) for slot in sorted(self._open) if self._pending[slot] > 0]
        if todo:
            self.to_model.step_streams_pinned(self._cin, self.state_in, self.capacity, todo, self._min, self.max_packet, produced=self._made_in[:len(todo)],
                                              **self._in_kw)
            self.to_model.synchronize()
            # the launch has consumed every stream's samples: the counters follow it for all of them before anything can raise
            made_in = []
            for i, (slot, n, _, _) in enumerate(todo):
                made = int(self._made_in[i])
                if made != self.to_model.produced(self._consumed[slot], n):
                    raise RuntimeError(f"slot {slot}: the resampler made {made} samples of {n}, {self.to_model.produced(self._consumed[slot], n)} were due")
                made_in.append(made)
            for slot, n, _, _ in todo:
                self._consumed[slot] += n
                self._pending[slot] = 0
            # push() has checked that the inner ring holds them.  Should inner.push raise all the same, the exception leaves the pool
            # consistent - every counter describes what the resamplers and the inner pool hold - and the samples of that slot and of the
            # slots behind it in this tick are dropped: those streams go on with a gap
            for (slot, _, _, _), made in zip(todo, made_in):
                if made:
                    self.inner.push(slot, self._min[slot, :made])
                    self._fill[slot] += made
        launched = self.inner.tick()
        back = []
        for slot in sorted(self._open):
            y = self.inner.pull(slot)
            n = int(y.numel())
            if n:
                self._mout[slot, :n] = y
                self._fill[slot] -= n
                back.append((slot, n, slot * self._step, slot * self._client_cap))
        if back:
            self.to_client.step_streams_pinned(self._mout, self.state_out, self.capacity, back, self._cout, self._step, produced=self._made_out[:len(back)],
                                               **self._out_kw)
            self.to_client.synchronize()
            for i, (slot, _, _, _) in enumerate(back):
                made = int(self._made_out[i])
                if made:
                    self._ready[slot].append(self._cout[slot, :made].clone())
        return launched

    def pull(self, slot: int) -> Tensor:
        """The enhanced int16 samples at the client's rate made since the last pull (a copy; empty when there are none)."""
        self._check_open(slot)
        parts, self._ready[slot] = self._ready[slot], []
        return torch.cat(parts) if parts else torch.zeros(0, dtype=self._client_dtype)


class RingResampledPacketPool(ResampledPacketPool):
    """ResampledPacketPool with the two resamplers reading and writing the inner pool's rings themselves (Resampler.step_rings_pinned,
    fe_resample_rings_pinned): no model-rate audio is copied on the host, and a tick waits once.  The surface is ResampledPacketPool's -
    open, close, push, tick, pull, active, inner, to_model, to_client, state_in, state_out, the _make_pool / _make_resampler hooks - and
    `pool` names the inner pool's class: PacketPool, FamilyPacketPool or BacklogPacketPool, built with **pool_kwargs (meters=, backlog_hops=).
    Limits, meters, banks and backlogs are used through `inner`, whose slots are this pool's.
    It owns two page-locked client-rate staging buffers ([capacity, max_packet] in, [capacity, client_cap] out) and two page-locked
    `produced` tables, and NO model-rate staging.  tick():
      1. for every open slot with pending samples the host computes made = to_model.produced(consumed, n) and reserves `made` samples in the
         inner input ring (PacketPool._reserve_push; push() has checked that they fit); one to_model.step_rings_pinned launch from the flat
         client staging into inner.ring_in at the reserved ring positions - the outputs wrap with the ring;
      2. inner._enqueue(): the inner pool's descriptors, which see the samples of step 1, and its one or two launches;
      3. for every stream those advanced, one to_client.step_rings_pinned launch from inner.ring_out, hops * H samples at the stream's pull
         position, into the flat client staging;
      4. ONE synchronize();
      5. inner._complete() and the inner pull counters (PacketPool._reserve_pull);
      6. both `produced` tables against the host's predictions: RuntimeError as ResampledPacketPool raises it, the counters describing what
         the launches consumed;
      7. the ready client-rate samples are appended per slot.
    All launches are on the current stream, and no descriptor depends on a device result: how many samples a stream emits for its next n is a
    host function (fe_resampler_produced), and the hop schedule follows from host counters.
    The contract: for the same sequence of open / push / tick / pull / close calls every pull() returns the int16 samples
    ResampledPacketPool returns, bit for bit, tick() returns the same list, and state_in / state_out hold the same rows - both pools round to
    int16 at the model's rate, the resampler is packetisation-exact, and the hop schedule is a function of host counters only.
    client_format="ulaw" / "alaw" (ResampledPacketPool's keyword): G.711 bytes in and out, the same bytes ResampledPacketPool returns.
    Not here: device-resident rings; the filter fused into the frame kernels' stream_sample / stream_store_row; move / resize / export of a
    resampled pool; a flush on close(); G.711 straight into a PacketPool at the model's rate; G.722 and other codecs."""

    def __init__(self, engine: Engine, capacity: int, ring_hops: int, client_rate: int, T_max: int = 1, max_packet: Optional[int] = None, *,
                 model_rate: int = 16000, client_format: str = "s16", pool=PacketPool, **pool_kwargs):
        self._set_client_format(client_format)
        client_rate, model_rate = operator.index(client_rate), operator.index(model_rate)
        if client_rate == model_rate:
            raise ValueError(f"client_rate {client_rate} is the model's rate: there is nothing to resample, use PacketPool")
        device = getattr(engine, "device", None)
        self.client_rate, self.model_rate = client_rate, model_rate
        self.to_model = self._make_resampler(client_rate, model_rate, device)
        self.to_client = self._make_resampler(model_rate, client_rate, device)
        self.inner = self._make_pool(engine, capacity, ring_hops, T_max, pool, **pool_kwargs)
        self.capacity = int(capacity)
        # model-rate samples a slot advances per tick at most: T_max hops, or a backlog launch's
        step = max(int(self.inner.T_max), int(getattr(self.inner, "backlog_hops", 0))) * int(self.inner.H)
        if max_packet is None:                                             # what an ordinary tick can take away, at the client's rate
            max_packet = -(-int(self.inner.T_max) * int(self.inner.H) * client_rate // model_rate)
        self.max_packet = operator.index(max_packet)
        if self.max_packet < 1:
            raise ValueError("max_packet must be at least 1")
        self._client_cap = self.to_client.out_count(step) + 1             # client-rate samples of one tick's output at most
        self._step = step
        self.state_in = self.to_model.new_state(self.capacity)
        self.state_out = self.to_client.new_state(self.capacity)
        self._cin = self.to_model.new_pinned(self.capacity, self.max_packet, dtype=self._client_dtype)
        self._cout = self.to_client.new_pinned(self.capacity, self._client_cap, dtype=self._client_dtype)
        self._made_in = self.to_model.new_pinned(self.capacity, dtype=torch.int32)
        self._made_out = self.to_client.new_pinned(self.capacity, dtype=torch.int32)
        self._pending = [0] * self.capacity          # client-rate samples waiting in _cin
        self._consumed = [0] * self.capacity         # client-rate samples the resampler to the model's rate has consumed
        self._fill = [0] * self.capacity             # model-rate samples in the inner pool's rings: reserved and not yet pulled
        self._returned = [0] * self.capacity         # model-rate samples the resampler to the client's rate has consumed
        self._ready: List[List[Tensor]] = [[] for _ in range(self.capacity)]
        self._open = set()

    @staticmethod
    def _make_pool(engine, capacity, ring_hops, T_max, pool=PacketPool, **pool_kwargs) -> PacketPool:
        return pool(engine, capacity, ring_hops, T_max=T_max, **pool_kwargs)

    def _fresh(self, slot: int) -> None:
        super()._fresh(slot)
        self._returned[slot] = 0

    def tick(self) -> List[Tuple[int, int, int, int]]:
        """The seven steps above: up to three launches (four with a backlog) and one wait.  Returns what inner.tick() would have returned."""
        inner, ring = self.inner, self.inner.ring
        todo, due_in = [], []
        for slot in sorted(self._open):
            n = self._pending[slot]
            if n > 0:
                made = self.to_model.produced(self._consumed[slot], n)
                pos = inner._reserve_push(slot, made)                     # (push() has checked that the ring holds them)
                todo.append((slot, n, slot * self.max_packet, slot * ring, self.max_packet, 0, ring, pos))
                due_in.append(made)
        if todo:
            self.to_model.step_rings_pinned(self._cin, self.state_in, self.capacity, todo, inner.ring_in, self.max_packet,
                                            produced=self._made_in[:len(todo)], **self._in_kw)
        launched = inner._enqueue()
        back = [(slot, hops * inner.H, slot * ring, slot * self._client_cap, ring, inner._pulled[slot] % ring, self._client_cap, 0)
                for slot, hops, _, _ in sorted(launched)]
        due_out = [self.to_client.produced(self._returned[slot], n) for slot, n, *_ in back]
        if back:
            self.to_client.step_rings_pinned(inner.ring_out, self.state_out, self.capacity, back, self._cout, self._step,
                                             produced=self._made_out[:len(back)], **self._out_kw)
        if todo or launched:
            inner.engine.synchronize()
        inner._complete(launched)
        # the launches have consumed every stream's samples: the counters follow them for all streams before anything can raise
        for (slot, n, *_), made in zip(todo, due_in):
            self._consumed[slot] += n
            self._pending[slot] = 0
            self._fill[slot] += made
        for slot, n, *_ in back:
            inner._reserve_pull(slot)
            self._fill[slot] -= n
            self._returned[slot] += n
        for i, ((slot, n, *_), due) in enumerate(zip(todo, due_in)):
            made = int(self._made_in[i])
            if made != due:
                raise RuntimeError(f"slot {slot}: the resampler made {made} samples of {n}, {due} were due")
        for i, ((slot, n, *_), due) in enumerate(zip(back, due_out)):
            made = int(self._made_out[i])
            if made != due:
                raise RuntimeError(f"slot {slot}: the resampler made {made} samples of {n}, {due} were due")
            if made:
                self._ready[slot].append(self._cout[slot, :made].clone())
        return launched
