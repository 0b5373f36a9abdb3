"""StreamPool: streams that join and leave one state buffer (fe_step_slots / fe_state_reset_slots).

The pool owns a state buffer sized for `capacity` streams.  open() hands out a free slot and resets its state; close() frees it;
step() advances only the streams named, each reading and writing its own slot - no gather or scatter of state; step_host() does the
same for audio in page-locked host memory (fe_step_slots_pinned).  No threads, no queues: the caller decides which streams have a hop
ready on each tick."""
from __future__ import annotations

from typing import List, Optional, Sequence

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
