"""StreamPool: streams that join and leave one state buffer (fe_step_slots / fe_state_reset_slots).

The pool owns a state buffer sized for `capacity` streams.  open() hands out a free slot and resets its state; close() frees it;
step() advances only the streams named, each reading and writing its own slot - no gather or scatter of state; step_host() does the
same for audio in page-locked host memory (fe_step_slots_pinned).  No threads, no queues: the caller decides which streams have a hop
ready on each tick.

PacketPool: a StreamPool for PACKET audio - int16 PCM that arrives in pieces of any length (10 or 20 ms packets against a hop of 256
samples, with network jitter).  push() copies a packet into the stream's page-locked ring, tick() is ONE fe_step_streams_pinned launch in
which every stream advances by the whole hops it has, pull() returns the enhanced PCM.  The kernel reads and writes the rings themselves."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import torch
from torch import Tensor

from .engine import Engine


class StreamPool:
    def __init__(self, engine: Engine, capacity: int):
        if capacity < 1:
            raise ValueError("capacity must be at least 1")
        self.engine = engine
        self.capacity = int(capacity)
        self.state = engine.new_state(self.capacity)
        self._free: List[int] = list(range(self.capacity - 1, -1, -1))      # popped from the end: lowest slot first
        self._open = set()

    @property
    def active(self) -> List[int]:
        return sorted(self._open)

    def open(self) -> int:
        """A free slot, its state reset (what a fresh fe_state_init leaves)."""
        if not self._free:
            raise RuntimeError(f"all {self.capacity} slots are open")
        slot = self._free.pop()
        self.engine.reset_slots(self.state, self.capacity, [slot])
        self._open.add(slot)
        return slot

    def close(self, slot: int) -> None:
        if slot not in self._open:
            raise ValueError(f"slot {slot} is not open")
        self._open.remove(slot)
        self._free.append(slot)

    def step(self, slots: Sequence[int], wav_in: Tensor, wav_out: Optional[Tensor] = None, T: int = 1) -> Tensor:
        """wav_in [n, T*H] (row i: stream slots[i]) -> wav_out [n, T*H]; the other streams' state is untouched."""
        for s in slots:
            if s not in self._open:
                raise ValueError(f"slot {s} is not open")
        return self.engine.step_slots(wav_in, self.state, self.capacity, list(slots), wav_out=wav_out, T=T)

    def step_host(self, slots: Sequence[int], wav_in: Tensor, wav_out: Optional[Tensor] = None, T: int = 1) -> Tensor:
        """step() for audio in page-locked HOST memory (fe_step_slots_pinned): wav_in [n, T*H] pinned -> wav_out [n, T*H] pinned
        (allocated when None), in one launch.  Asynchronous on the current stream: synchronise it before reading wav_out."""
        for s in slots:
            if s not in self._open:
                raise ValueError(f"slot {s} is not open")
        return self.engine.step_slots_pinned(wav_in, self.state, self.capacity, list(slots), wav_out=wav_out, T=T)


class PacketPool(StreamPool):
    """Streams fed by int16 PCM packets of any length.  Every slot has an input and an output ring of ring_hops * H samples in page-locked
    host memory; a stream's sample k lives at ring position k mod (ring_hops * H) of both.  Between the oldest sample not yet pulled and
    the newest one pushed a stream may hold one ring of samples: push() refuses what would overwrite them.  No threads, no queues."""

    def __init__(self, engine: Engine, capacity: int, ring_hops: int, T_max: int = 1):
        super().__init__(engine, capacity)
        if ring_hops < 1 or T_max < 1:
            raise ValueError("ring_hops and T_max must be at least 1")
        self.H = int(engine.cfg.hop_size)
        self.ring = int(ring_hops) * self.H
        self.T_max = int(T_max)
        self.ring_in = engine.new_pinned(self.capacity, self.ring, dtype=torch.int16)
        self.ring_out = engine.new_pinned(self.capacity, self.ring, dtype=torch.int16)
        # per slot, in samples since open(): pushed >= stepped (a multiple of H) >= pulled
        self._pushed = [0] * self.capacity
        self._stepped = [0] * self.capacity
        self._pulled = [0] * self.capacity

    def open(self) -> int:
        slot = super().open()
        self._pushed[slot] = self._stepped[slot] = self._pulled[slot] = 0
        return slot

    def _check_open(self, slot: int) -> None:
        if slot not in self._open:
            raise ValueError(f"slot {slot} is not open")

    def push(self, slot: int, pcm) -> None:
        """Append a packet: a 1-D int16 array or tensor of any length.  The copy wraps at the ring end."""
        self._check_open(slot)
        x = torch.as_tensor(pcm)
        if x.dim() != 1 or x.dtype != torch.int16:
            raise ValueError(f"a packet is a 1-D int16 array, got {x.dtype} {tuple(x.shape)}")
        n, w = x.numel(), self._pushed[slot]
        if w + n - self._pulled[slot] > self.ring:
            raise OverflowError(f"slot {slot}: {n} samples do not fit - the ring holds {self.ring} samples between pull() and push(), "
                                f"{w - self._pulled[slot]} are in it")
        pos = w % self.ring
        first = min(n, self.ring - pos)
        self.ring_in[slot, pos:pos + first] = x[:first]
        if first < n:
            self.ring_in[slot, :n - first] = x[first:]
        self._pushed[slot] = w + n

    def tick(self) -> List[Tuple[int, int, int, int]]:
        """One launch for every open stream with at least one complete hop: each advances min(complete hops, hops up to the ring end,
        T_max); the rest waits for the next tick.  Waits for the launch (the rings are host memory the caller reads next).  Returns the
        descriptors (slot, hops, in_offset, out_offset) it launched - [] when no stream had a hop, and then nothing is launched."""
        desc = []
        for slot in sorted(self._open):
            pos = self._stepped[slot] % self.ring
            hops = min((self._pushed[slot] - self._stepped[slot]) // self.H, (self.ring - pos) // self.H, self.T_max)
            if hops > 0:
                off = slot * self.ring + pos
                desc.append((slot, hops, off, off))
        if not desc:
            return desc
        self.engine.step_streams_pinned(self.ring_in, self.state, self.capacity, desc, self.ring_out, T_max=self.T_max)
        self.engine.synchronize()
        for slot, hops, _, _ in desc:
            self._stepped[slot] += hops * self.H
        return desc

    def pull(self, slot: int) -> Tensor:
        """The enhanced int16 samples produced since the last pull (a copy; empty when there are none)."""
        self._check_open(slot)
        r, n = self._pulled[slot], self._stepped[slot] - self._pulled[slot]
        pos = r % self.ring
        first = min(n, self.ring - pos)
        out = torch.cat([self.ring_out[slot, pos:pos + first], self.ring_out[slot, :n - first]])
        self._pulled[slot] = r + n
        return out
