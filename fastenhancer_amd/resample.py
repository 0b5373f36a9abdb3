"""Resampler: one fe_resampler (C ABI) on one GPU - polyphase resampling of whole signals and of packet streams.

The filter, the index arithmetic and the streaming rule are the library's (include/fastenhancer_hip.h, "Audio at another sample rate"):
scipy.signal.resample_poly(x, up, down) with its defaults, in fp32 on the GPU.  PyTorch is used for device memory and streams only."""
from __future__ import annotations

import operator
from ctypes import POINTER, byref, c_double, c_void_p, cast
from typing import List, Optional

import torch
from torch import Tensor

from . import _lib
from .engine import _ptr, _stream


def _fmt(t: Tensor) -> int:
    return _lib.FE_AUDIO_S16 if t.dtype == torch.int16 else _lib.FE_AUDIO_F32


_LAW_FORMATS = {"ulaw": _lib.FE_AUDIO_ULAW, "alaw": _lib.FE_AUDIO_ALAW}


def _check_law(what: str, law) -> None:
    """in_format= / out_format=: None (the format is the tensor's dtype) or a G.711 law"""
    if law is not None and law not in _LAW_FORMATS:
        raise ValueError(f"{what} must be None, 'ulaw' or 'alaw', got {law!r}")


def _law_fmt(what: str, t: Tensor, law) -> int:
    """the format code of tensor t under `law`: a law's bytes are a uint8 tensor"""
    if law is None:
        return _fmt(t)
    if t.dtype != torch.uint8:
        raise ValueError(f"{what}: G.711 {law} is one byte per sample - the tensor must be torch.uint8, got {t.dtype}")
    return _LAW_FORMATS[law]


class Resampler:
    """sr_in -> sr_out.  Creation and every query work without a GPU; the calls that resample need a CUDA device."""

    def __init__(self, sr_in: int, sr_out: int, device: Optional[torch.device] = None):
        self.lib = _lib.load()
        self.sr_in, self.sr_out = operator.index(sr_in), operator.index(sr_out)
        self.device = torch.device(device) if device is not None else None
        if self.device is not None and self.device.type == "cuda" and self.device.index is None and torch.cuda.is_available():
            self.device = torch.device("cuda", torch.cuda.current_device())
        self._h = c_void_p()
        _lib.check(self.lib.fe_resampler_create(self.sr_in, self.sr_out, byref(self._h)), "fe_resampler_create")
        self.up = int(self.lib.fe_resampler_up(self._h))
        self.down = int(self.lib.fe_resampler_down(self._h))
        self.taps_per_output = int(self.lib.fe_resampler_taps_per_output(self._h))
        self.half_len = int(self.lib.fe_resampler_half_len(self._h))
        self.state_floats = int(self.lib.fe_resampler_state_floats(self._h))
        self._desc_pin: Optional[Tensor] = None      # page-locked staging of ring descriptors (_upload_desc)
        self._desc_event = None

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            try:
                self.lib.fe_resampler_destroy(h)
            except Exception:
                pass
            self._h = None          # (not c_void_p(): at interpreter shutdown the module's globals may be gone)

    # ------------------------------------------------------------------ queries (no GPU)
    def taps(self) -> Tensor:
        """the 2 * half_len + 1 taps h = up * firwin(...) as designed, float64"""
        n = 2 * self.half_len + 1
        out = torch.zeros(n, dtype=torch.float64)
        got = self.lib.fe_resampler_taps(self._h, cast(c_void_p(out.data_ptr()), POINTER(c_double)), n)
        if got != n:
            _lib.check(got if got < 0 else -1, "fe_resampler_taps")
        return out

    def out_count(self, n_in: int) -> int:
        """outputs of a whole-signal call on n_in samples: ceil(n_in * up / down)"""
        return int(self.lib.fe_resampler_out_count(self._h, int(n_in)))

    def produced(self, consumed: int, n_in: int) -> int:
        """outputs a stream that has consumed `consumed` samples emits for its next n_in"""
        return int(self.lib.fe_resampler_produced(self._h, int(consumed), int(n_in)))

    @property
    def latency_samples(self) -> float:
        """the stream's latency in input samples: half_len / up"""
        return self.half_len / self.up

    def last_kernel(self) -> str:
        return self.lib.fe_resampler_last_kernel(self._h).decode()

    # ------------------------------------------------------------------ compute
    def _require_gpu(self):
        if self.device is None or self.device.type != "cuda" or not torch.cuda.is_available():
            raise _lib.FEError("the resampler needs a GPU device (no CPU fallback); got device=%r" % (self.device,))

    def __call__(self, x: Tensor, out_dtype=None, *, in_format=None, out_format=None) -> Tensor:
        """x: float32 or int16 [B, L] (or [L]) on the device -> [B, out_count(L)] of out_dtype (default: x's).
        in_format="ulaw" / "alaw": x is uint8 G.711 bytes (out_dtype then defaults to int16).  out_format="ulaw" / "alaw": the output is
        uint8 G.711 bytes (out_dtype must be left alone).  See fastenhancer_amd.g711 for making and reading such bytes."""
        _check_law("in_format", in_format)
        _check_law("out_format", out_format)
        if in_format is not None:
            if not isinstance(x, Tensor) or x.dim() not in (1, 2) or x.numel() == 0:
                raise ValueError("x must be a non-empty tensor [B, L] or [L]")
            _law_fmt("x", x, in_format)
        elif not isinstance(x, Tensor) or x.dtype not in (torch.float32, torch.int16) or x.dim() not in (1, 2) or x.numel() == 0:
            raise ValueError("x must be a non-empty float32 or int16 tensor [B, L] or [L]")
        if out_format is not None:
            if out_dtype not in (None, torch.uint8):
                raise ValueError(f"out_format={out_format!r} makes the output torch.uint8: leave out_dtype alone (got {out_dtype})")
            out_dtype = torch.uint8
        else:
            out_dtype = (torch.int16 if in_format is not None else x.dtype) if out_dtype is None else out_dtype
            if out_dtype not in (torch.float32, torch.int16):
                raise ValueError("out_dtype must be float32 or int16")
        self._require_gpu()
        rows = x.to(self.device).reshape(-1, x.shape[-1]).contiguous()
        B, n_in = rows.shape
        n_out = self.out_count(n_in)
        out = torch.empty(B, n_out, dtype=out_dtype, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.fe_resample(self._h, _ptr(rows), n_in, _law_fmt("x", rows, in_format), n_in, _ptr(out), n_out,
                                            _law_fmt("out", out, out_format), B, _stream(self.device)), "fe_resample")
        return out[0] if x.dim() == 1 else out

    def new_state(self, capacity: int) -> Tensor:
        """[capacity, state_floats] zeros on the device: every row a fresh stream.  A row is plain data - hist[K - 1] oldest first, the
        consumed count as two 32-bit words, padding to 4 floats: copy a row to move a stream, zero it to restart one."""
        self._require_gpu()
        return torch.zeros(int(capacity), self.state_floats, dtype=torch.float32, device=self.device)

    @staticmethod
    def pack_desc(desc) -> Tensor:
        """[(slot, n_in, in_offset, out_offset), ...] -> a CPU int32 tensor [n, 6], the memory image of n fe_resample_desc"""
        rows = [tuple(operator.index(v) for v in d) for d in desc]
        if any(len(r) != 4 for r in rows):
            raise ValueError("a stream descriptor is (slot, n_in, in_offset, out_offset)")
        arr = (_lib.fe_resample_desc * max(len(rows), 1))(*[_lib.fe_resample_desc(*r) for r in rows])
        words = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.int32).view(-1, 6)
        return words[:len(rows)].clone()

    def _desc_tensor(self, desc, capacity: int, n_in_max: int, in_count: int) -> Tensor:
        """A CUDA int32 tensor [n, 6] is passed through unchecked (the kernel checks every descriptor itself); a list of
        (slot, n_in, in_offset, out_offset) is checked here first - slots in [0, capacity) without duplicates, 0 <= n_in <= n_in_max, the
        input range inside its buffer (the output range depends on the stream's count: the kernel's to check) - and copied to the device."""
        if isinstance(desc, Tensor):
            if desc.dtype != torch.int32 or desc.dim() != 2 or desc.shape[1] != 6 or not desc.is_contiguous():
                raise ValueError("a descriptor tensor must be a contiguous int32 tensor [n, 6] (Resampler.pack_desc)")
            if desc.is_cuda:
                return desc
            self._require_gpu()
            return desc.to(self.device)
        rows = [tuple(operator.index(v) for v in d) for d in desc]
        if not 1 <= len(rows) <= capacity:
            raise ValueError(f"{len(rows)} streams for a capacity of {capacity}")
        for slot, n_in, i0, o0 in rows:
            if not 0 <= slot < capacity:
                raise ValueError(f"slot {slot} is outside [0, {capacity})")
            if not 0 <= n_in <= n_in_max:
                raise ValueError(f"n_in {n_in} is outside [0, {n_in_max}]")
            if i0 < 0 or i0 + n_in > in_count:
                raise ValueError(f"slot {slot}: input range [{i0}, {i0 + n_in}) is outside [0, {in_count})")
            if o0 < 0:
                raise ValueError(f"slot {slot}: output offset {o0} is negative")
        if len({r[0] for r in rows}) != len(rows):
            raise ValueError("duplicate slots")
        self._require_gpu()
        return self.pack_desc(rows).to(self.device)

    @staticmethod
    def pack_ring_desc(rows) -> Tensor:
        """[(slot, n_in, in_base, out_base, in_len, in_pos, out_len, out_pos), ...] -> a CPU int32 tensor [n, 10], the memory image of n
        fe_resample_ring_desc"""
        rows = [tuple(operator.index(v) for v in d) for d in rows]
        if any(len(r) != 8 for r in rows):
            raise ValueError("a ring descriptor is (slot, n_in, in_base, out_base, in_len, in_pos, out_len, out_pos)")
        arr = (_lib.fe_resample_ring_desc * max(len(rows), 1))(*[_lib.fe_resample_ring_desc(*r) for r in rows])
        words = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.int32).view(-1, 10)
        return words[:len(rows)].clone()

    @staticmethod
    def check_ring_desc(rows, capacity: int, n_in_max: int, in_count: int, out_count: int) -> None:
        """The kernel's rules for ring descriptors, on the host: where the kernel would skip the stream without a word, a ValueError.  Slots in
        [0, capacity) without duplicates, 0 <= n_in <= n_in_max, each ring at least one element long with its position inside it and the
        whole of it inside its buffer, n_in <= in_len.  (That the outputs fit, p <= out_len, depends on the stream's count: the kernel's to
        check, and `produced` says what it found.)"""
        if not 1 <= len(rows) <= capacity:
            raise ValueError(f"{len(rows)} streams for a capacity of {capacity}")
        for slot, n_in, in_base, out_base, in_len, in_pos, out_len, out_pos in rows:
            if not 0 <= slot < capacity:
                raise ValueError(f"slot {slot} is outside [0, {capacity})")
            if not 0 <= n_in <= n_in_max:
                raise ValueError(f"n_in {n_in} is outside [0, {n_in_max}]")
            for what, base, length, pos, count in (("input", in_base, in_len, in_pos, in_count), ("output", out_base, out_len, out_pos, out_count)):
                if length < 1:
                    raise ValueError(f"slot {slot}: the {what} ring's length {length} is less than 1")
                if not 0 <= pos < length:
                    raise ValueError(f"slot {slot}: the {what} ring's position {pos} is outside [0, {length})")
                if base < 0 or base + length > count:
                    raise ValueError(f"slot {slot}: the {what} ring [{base}, {base + length}) is outside [0, {count})")
            if n_in > in_len:
                raise ValueError(f"slot {slot}: n_in {n_in} is more than the input ring's length {in_len}")
        if len({r[0] for r in rows}) != len(rows):
            raise ValueError("duplicate slots")

    def _ring_desc_tensor(self, desc, capacity: int, n_in_max: int, in_count: int, out_count: int) -> Tensor:
        """_desc_tensor for ring descriptors: a CUDA int32 tensor [n, 10] passes unchecked, a list is checked (check_ring_desc) and copied"""
        if isinstance(desc, Tensor):
            if desc.dtype != torch.int32 or desc.dim() != 2 or desc.shape[1] != 10 or not desc.is_contiguous():
                raise ValueError("a ring descriptor tensor must be a contiguous int32 tensor [n, 10] (Resampler.pack_ring_desc)")
            if desc.is_cuda:
                return desc
            self._require_gpu()
            return desc.to(self.device)
        rows = [tuple(operator.index(v) for v in d) for d in desc]
        if any(len(r) != 8 for r in rows):
            raise ValueError("a ring descriptor is (slot, n_in, in_base, out_base, in_len, in_pos, out_len, out_pos)")
        self.check_ring_desc(rows, capacity, n_in_max, in_count, out_count)
        self._require_gpu()
        return self._upload_desc(self.pack_ring_desc(rows))

    def _upload_desc(self, words: Tensor) -> Tensor:
        """CPU descriptor words -> a device tensor, without waiting for the stream (a copy from pageable memory would wait for everything
        launched before it): staged in a page-locked buffer of the handle's and copied asynchronously on the current stream.  The event
        keeps the next call from rewriting the staging buffer before this copy has read it."""
        n = words.shape[0]
        if self._desc_event is not None:
            self._desc_event.synchronize()
        if self._desc_pin is None or self._desc_pin.shape[0] < n:
            self._desc_pin = torch.empty(max(n, 16), words.shape[1], dtype=torch.int32).pin_memory()
        self._desc_pin[:n].copy_(words)
        with torch.cuda.device(self.device):
            d = self._desc_pin[:n].to(self.device, non_blocking=True)
            if self._desc_event is None:
                self._desc_event = torch.cuda.Event()
            self._desc_event.record(torch.cuda.current_stream(self.device))
        return d

    def _step_streams(self, x: Tensor, state: Tensor, capacity: int, desc, out: Tensor, n_in_max: int, produced: Optional[Tensor], pinned: bool,
                      rings: bool = False, in_format=None, out_format=None):
        name = ("fe_resample_rings" if rings else "fe_resample_streams") + ("_pinned" if pinned else "")
        _check_law("in_format", in_format)
        _check_law("out_format", out_format)
        for what, t, law in (("x", x, in_format), ("out", out, out_format)):
            if law is not None:
                if not isinstance(t, Tensor) or not t.is_contiguous() or t.numel() == 0:
                    raise ValueError(f"{what} must be a contiguous, non-empty tensor")
                _law_fmt(what, t, law)
            elif not isinstance(t, Tensor) or t.dtype not in (torch.float32, torch.int16) or not t.is_contiguous() or t.numel() == 0:
                raise ValueError(f"{what} must be a contiguous, non-empty float32 or int16 tensor")
            if pinned and (t.device.type != "cpu" or not t.is_pinned()):
                raise ValueError(f"{what} must be a CPU tensor in page-locked memory (pin_memory())")
            if not pinned and not t.is_cuda:
                raise ValueError(f"{what} must be a device tensor ({name}_pinned takes page-locked host memory)")
        if n_in_max < 1:
            raise ValueError("n_in_max must be at least 1")
        n_desc = desc.shape[0] if isinstance(desc, Tensor) else len(desc)
        if produced is not None:
            if not isinstance(produced, Tensor) or produced.dtype != torch.int32 or tuple(produced.shape) != (n_desc,) or not produced.is_contiguous():
                raise ValueError(f"produced must be a contiguous int32 tensor [{n_desc}]")
            if not produced.is_cuda and not (produced.device.type == "cpu" and produced.is_pinned()):
                raise ValueError("produced must be a device tensor or a CPU tensor in page-locked memory (pin_memory())")
        d = self._ring_desc_tensor(desc, capacity, n_in_max, x.numel(), out.numel()) if rings else self._desc_tensor(desc, capacity, n_in_max, x.numel())
        self._require_gpu()
        if not (isinstance(state, Tensor) and state.is_cuda and state.dtype == torch.float32 and state.is_contiguous()
                and state.numel() == capacity * self.state_floats):
            raise ValueError(f"state must be a contiguous float32 device tensor of {capacity} x {self.state_floats} floats (new_state)")
        with torch.cuda.device(self.device):
            _lib.check(getattr(self.lib, name)(self._h, _ptr(x), x.numel(), _law_fmt("x", x, in_format), _ptr(state), int(capacity), _ptr(d), _ptr(out),
                                               out.numel(), _law_fmt("out", out, out_format), _ptr(produced), d.shape[0], int(n_in_max),
                                               _stream(self.device)), name)
        self._keep = (d, x, out, produced)       # (alive until the next call - the launch is asynchronous)
        return out

    def step_streams(self, x: Tensor, state: Tensor, capacity: int, desc, out: Tensor, n_in_max: int, produced: Optional[Tensor] = None, *,
                         in_format=None, out_format=None) -> Tensor:
        """fe_resample_streams: every stream of `desc` - (slot, n_in, in_offset, out_offset), or a CUDA int32 tensor [n, 6] - consumes its n_in
        samples from the flat device buffer x and writes the outputs that become due to the flat device buffer `out` (either float32 or
        int16, independently).  state: new_state(capacity).  produced: an int32 tensor [n] (device or page-locked), each stream's output count.
        in_format / out_format: None - the format is the tensor's dtype - or "ulaw" / "alaw": that side is a uint8 tensor of G.711 bytes
        (one byte per sample: counts and offsets are bytes), decoded or encoded by the kernel.  The same two keywords on the three forms below."""
        return self._step_streams(x, state, capacity, desc, out, n_in_max, produced, pinned=False, in_format=in_format, out_format=out_format)

    def step_streams_pinned(self, x: Tensor, state: Tensor, capacity: int, desc, out: Tensor, n_in_max: int, produced: Optional[Tensor] = None, *,
                                in_format=None, out_format=None) -> Tensor:
        """fe_resample_streams_pinned: step_streams with x / out in page-locked HOST memory.  Asynchronous on the current stream: synchronise
        it before reading out (or a pinned `produced`) or rewriting x."""
        return self._step_streams(x, state, capacity, desc, out, n_in_max, produced, pinned=True, in_format=in_format, out_format=out_format)

    def step_rings(self, x: Tensor, state: Tensor, capacity: int, desc, out: Tensor, n_in_max: int, produced: Optional[Tensor] = None, *,
                       in_format=None, out_format=None) -> Tensor:
        """fe_resample_rings: step_streams for streams whose samples live in rings inside x and out.  desc: a list of
        (slot, n_in, in_base, out_base, in_len, in_pos, out_len, out_pos) - sample i of the packet is x[in_base + (in_pos + i) % in_len],
        output m of the call out[out_base + (out_pos + m) % out_len]; checked on the host (check_ring_desc: ValueError where the kernel
        would skip the stream) - or a CUDA int32 tensor [n, 10] (pack_ring_desc), which the kernel alone checks.  A flat buffer is pos = 0
        with len at least the count."""
        return self._step_streams(x, state, capacity, desc, out, n_in_max, produced, pinned=False, rings=True, in_format=in_format, out_format=out_format)

    def step_rings_pinned(self, x: Tensor, state: Tensor, capacity: int, desc, out: Tensor, n_in_max: int, produced: Optional[Tensor] = None, *,
                              in_format=None, out_format=None) -> Tensor:
        """fe_resample_rings_pinned: step_rings with x / out in page-locked HOST memory - the rings of a PacketPool, for one.  Asynchronous on
        the current stream: synchronise it before reading out (or a pinned `produced`) or rewriting x."""
        return self._step_streams(x, state, capacity, desc, out, n_in_max, produced, pinned=True, rings=True, in_format=in_format, out_format=out_format)

    def new_pinned(self, *shape: int, dtype=torch.float32) -> Tensor:
        self._require_gpu()
        return torch.zeros(*shape, dtype=dtype).pin_memory()

    def synchronize(self) -> None:
        self._require_gpu()
        torch.cuda.current_stream(self.device).synchronize()
