"""Engine: one fe_handle (C ABI) on one GPU + torch-tensor convenience around it.

PyTorch is used for device memory and streams only; all arithmetic of the path
runs in libfastenhancer_hip.so."""
from __future__ import annotations

import ctypes
import operator
from ctypes import byref, c_char_p, c_int, c_size_t, c_void_p
from typing import Dict, List, Mapping, Optional, Tuple

import torch
from torch import Tensor

from . import _lib
from .config import FEConfig
from .family import family_of, packet_chunk_on_request, views


def _ptr(t: Optional[Tensor]) -> c_void_p:
    return c_void_p(0 if t is None else t.data_ptr())


def _stream(device: torch.device) -> c_void_p:
    return c_void_p(torch.cuda.current_stream(device).cuda_stream)


class Engine:
    """Owns the native handle for one model shape on one device."""

    def __init__(self, cfg: FEConfig, device: Optional[torch.device] = None):
        self.lib = _lib.load()
        self.cfg = cfg
        self.device = torch.device(device) if device is not None else None
        if self.device is not None and self.device.type == "cuda" and self.device.index is None and torch.cuda.is_available():
            # torch.device('cuda') != torch.device('cuda:0'): keep one spelling, the indexed one tensors report
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.family = family_of(cfg)
        c = _lib.fe_config()
        c.arch = self.family.arch
        c.n_fft, c.hop_size, c.win_size = cfg.n_fft, cfg.hop_size, cfg.win_size
        c.input_compression = cfg.input_compression
        self.family.fill_config(c, cfg)       # (may raise: no kernel compiled for this architecture)
        self._h = c_void_p()
        if self.device is not None and self.device.type == "cuda":
            with torch.cuda.device(self.device):
                _lib.check(self.lib.fe_create(byref(c), byref(self._h)), "fe_create")
        else:
            _lib.check(self.lib.fe_create(byref(c), byref(self._h)), "fe_create")
        self.weight_floats = int(self.lib.fe_weight_floats(self._h))
        self.sections = self._read_sections()
        self.flops_per_frame = float(self.lib.fe_flops_per_frame(self._h))
        self.loaded = False

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            try:
                self.lib.fe_destroy(h)
            except Exception:
                pass
            self._h = c_void_p()

    # ------------------------------------------------------------------ weights
    def _read_sections(self) -> List[Tuple[str, int, int]]:
        out = []
        for i in range(self.lib.fe_weight_sections(self._h)):
            name, off, cnt = c_char_p(), c_size_t(), c_size_t()
            _lib.check(self.lib.fe_weight_section(self._h, i, byref(name), byref(off), byref(cnt)), "fe_weight_section")
            out.append((name.value.decode(), int(off.value), int(cnt.value)))
        return out

    def make_blob(self, state_dict: Mapping[str, Tensor], strict: bool = True) -> Tensor:
        """reference checkpoint (training or fused form) -> flat fp32 blob on the CPU."""
        fused = self.family.fold(state_dict, self.cfg)
        self.family.check(fused, self.cfg, strict=strict)
        blob = torch.zeros(self.weight_floats, dtype=torch.float32)
        for name, off, cnt in self.sections:
            t = fused[name].contiguous().reshape(-1)
            assert t.numel() == cnt, (name, t.numel(), cnt)
            blob[off:off + cnt] = t
        return blob

    @property
    def weight_banks(self) -> int:
        """fe_weight_banks: checkpoints the handle holds side by side (1 unless set_weight_banks asked for more)"""
        return int(self.lib.fe_weight_banks(self._h))

    def set_weight_banks(self, n: int) -> None:
        """fe_set_weight_banks: room for n checkpoints of this shape (1 .. 64), bank 0 being what every other step reads; the banks that
        survive keep their contents.  Load-time work: it may synchronise the current stream and must not be called inside a capture."""
        n = operator.index(n)
        if self.device is not None and self.device.type == "cuda" and torch.cuda.is_available():
            with torch.cuda.device(self.device):
                _lib.check(self.lib.fe_set_weight_banks(self._h, n, _stream(self.device)), "fe_set_weight_banks")
        else:       # (no GPU: the arguments are still checked; nothing is loaded, so there is nothing to move)
            _lib.check(self.lib.fe_set_weight_banks(self._h, n, None), "fe_set_weight_banks")

    def _bank(self, bank) -> int:
        bank = operator.index(bank)
        if not 0 <= bank < self.weight_banks:
            raise ValueError(f"bank {bank} is outside [0, {self.weight_banks}) (set_weight_banks)")
        return bank

    def load_blob(self, blob_dev: Tensor, bank: int = 0):
        """fe_load_weights_bank: the blob into bank `bank`, in place (bank 0: fe_load_weights)"""
        bank = self._bank(bank)
        self._require_gpu()
        assert blob_dev.is_cuda and blob_dev.dtype == torch.float32 and blob_dev.is_contiguous()
        with torch.cuda.device(self.device):
            if bank == 0:
                _lib.check(self.lib.fe_load_weights(self._h, _ptr(blob_dev), blob_dev.numel(), _stream(self.device)), "fe_load_weights")
            else:
                _lib.check(self.lib.fe_load_weights_bank(self._h, bank, _ptr(blob_dev), blob_dev.numel(), _stream(self.device)), "fe_load_weights_bank")
        if bank == 0:
            self.loaded = True

    def pack_blob(self, blob_cpu: Tensor) -> Tensor:
        """the buffer the kernels read, packed on the CPU from a make_blob() blob: what load_blob uploads (fe_debug_pack_weights; needs no GPU)."""
        assert not blob_cpu.is_cuda and blob_cpu.dtype == torch.float32 and blob_cpu.is_contiguous()
        n = c_size_t()
        _lib.check(self.lib.fe_debug_pack_weights(self._h, _ptr(blob_cpu), blob_cpu.numel(), None, 0, byref(n)), "fe_debug_pack_weights")
        out = torch.empty(n.value, dtype=torch.float32)
        _lib.check(self.lib.fe_debug_pack_weights(self._h, _ptr(blob_cpu), blob_cpu.numel(), _ptr(out), out.numel(), byref(n)), "fe_debug_pack_weights")
        return out

    def load_state_dict(self, state_dict: Mapping[str, Tensor], strict: bool = True, bank: int = 0):
        bank = self._bank(bank)
        blob = self.make_blob(state_dict, strict=strict)
        self.load_blob(blob.to(self.device), bank)

    # ------------------------------------------------------------------ state
    def _require_gpu(self):
        if self.device is None or self.device.type != "cuda" or not torch.cuda.is_available():
            raise _lib.FEError("the FastEnhancer HIP path needs a GPU device (no CPU fallback); got device=%r" % (self.device,))

    def state_floats(self, B: int) -> int:
        return int(self.lib.fe_state_floats(self._h, B))

    def new_state(self, B: int) -> Tensor:
        self._require_gpu()
        return torch.zeros(self.state_floats(B), dtype=torch.float32, device=self.device)

    def init_state(self, state: Tensor, B: int) -> Tensor:
        """fe_state_init: `state` (sized for B streams) zeroed, and the engine's per-hop scratch sized for B streams - what step_pool, which
        allocates nothing, runs BSRNN's three-launch step on (step() grows that scratch itself on its first call)."""
        self._require_gpu()
        if not isinstance(state, Tensor) or not state.is_cuda or state.dtype != torch.float32 or not state.is_contiguous() or state.numel() != self.state_floats(B):
            raise ValueError(f"state must be a contiguous float32 device tensor of state_floats({B}) = {self.state_floats(B)} floats")
        with torch.cuda.device(self.device):
            _lib.check(self.lib.fe_state_init(self._h, _ptr(state), int(B), _stream(self.device)), "fe_state_init")
        return state

    def split_state(self, state: Tensor, B: int, head0: bool = False) -> List[Tensor]:
        """Views of the opaque state as the reference cache list [cache_stft [B,N-H], cache_istft [B,N-H], *the model's caches]
        (scripts/export_onnx.py:43-46).  The dptransformer variant's caches are copies unless head0 (family.py)."""
        n = B * self.cfg.cache_len
        return views(state[:2 * n], [(B, self.cfg.cache_len)] * 2) + self.family.split(self.cfg, state[2 * n:], B, head0)

    def model_state_order(self, caches: List[Tensor]) -> List[Tensor]:
        """the model's cache list (reference order) -> flat pieces in the order of the C ABI state (h ..., then the conv caches)"""
        return self.family.order(self.cfg, caches)

    def pack_state(self, caches: List[Tensor], B: int) -> Tensor:
        pieces = [t.reshape(-1) for t in caches[:2]] + self.model_state_order(list(caches[2:]))
        return torch.cat([t.to(torch.float32) for t in pieces]).contiguous()

    # ------------------------------------------------------------------ compute
    def _step(self, wav_in: Tensor, state: Tensor, wav_out: Optional[Tensor], T: int, capacity: Optional[int] = None, slots=None,
              pinned: bool = False, pool: bool = False) -> Tensor:
        """The streaming step behind step / step_slots / step_pool / step_pinned / step_slots_pinned.  slots (with capacity): the slot-indexed
        entry points, `state` sized for `capacity` streams; pinned: wav_in / wav_out are page-locked host memory instead of device memory;
        pool (slotted, device audio): fe_step_pool, the slotted step of every family, instead of fe_step_slots."""
        slotted = slots is not None
        H = self.cfg.hop_size
        if pinned:
            if not isinstance(wav_in, Tensor) or wav_in.dim() != 2:
                raise ValueError(f"wav_in must be a 2-D tensor [{'n' if slotted else 'B'}, T*H]")
            wav_in = self._pinned_audio("wav_in", wav_in, wav_in.shape[0], T)
            wav_out = self._pinned_audio("wav_out", wav_out, wav_in.shape[0], T)
        sl = self._slot_tensor(slots, capacity) if slotted else None
        self._require_gpu()
        n = wav_in.shape[0]
        if slotted:
            assert sl.numel() == n, (sl.numel(), n)
        if not pinned:
            assert wav_in.is_cuda and wav_in.dtype == torch.float32 and wav_in.stride(1) == 1 and wav_in.shape[1] == T * H
        assert (state.is_cuda or not pinned) and state.numel() == self.state_floats(capacity if slotted else n) and state.is_contiguous()
        if wav_out is None:
            wav_out = torch.empty(n, T * H, dtype=torch.float32, device=wav_in.device)
        name = "fe_step_pool" if pool else "fe_step" + ("_slots" if slotted else "") + ("_pinned" if pinned else "")
        args = [self._h, _ptr(wav_in), wav_in.stride(0) if n > 1 else T * H, _ptr(state)]
        args += [int(capacity), _ptr(sl)] if slotted else []
        args += [_ptr(wav_out), wav_out.stride(0) if n > 1 else T * H, n, T, _stream(self.device)]
        with torch.cuda.device(self.device):
            _lib.check(getattr(self.lib, name)(*args), name)
        # (alive until the next call - the launch is asynchronous: a copied slot list, the pinned audio)
        if slotted:
            self._slots_keep = sl
        if pinned:
            self._pinned_keep = (wav_in, wav_out)
        return wav_out

    def step(self, wav_in: Tensor, state: Tensor, wav_out: Optional[Tensor] = None, T: int = 1) -> Tensor:
        """wav_in [B, T*H] (row stride free) -> wav_out [B, T*H]; state updated in place."""
        return self._step(wav_in, state, wav_out, T)

    # ---- few streams, many hops: chunks on the time pipeline (fe_step_chunk)
    def chunk_work_floats(self, B: int, T: int) -> int:
        """fe_step_chunk_work_floats: floats of scratch step_chunk needs for at most B streams of at most T hops (0: none)."""
        return int(self.lib.fe_step_chunk_work_floats(self._h, int(B), int(T)))

    def step_chunk(self, wav_in: Tensor, state: Tensor, wav_out: Optional[Tensor] = None, T: Optional[int] = None, work: Optional[Tensor] = None) -> Tensor:
        """fe_step_chunk: step(wav_in, state, wav_out, T) with the T hops of each stream on the time pipeline - a recording, or a stream with
        a backlog.  wav_in [B, T*H] (row stride free; T defaults to wav_in.shape[1] // H) -> wav_out [B, T*H], which must not overlap wav_in;
        state updated in place.  Results agree with step() to fp32 rounding.  work: a float32 device tensor of at least
        chunk_work_floats(B, T) floats (the form for graph capture); None: a scratch tensor kept on the engine, grown when needed.
        BSRNN, FSPEN and LiSenNet are not pipelined here: step_backlog."""
        return self._chunk("fe_step_chunk", "chunk_work_floats", wav_in, state, wav_out, T, work)

    # ---- the same for every family with a streaming state (fe_step_backlog): BSRNN and FSPEN chunks on the time pipeline too
    def backlog_work_floats(self, B: int, T: int) -> int:
        """fe_step_backlog_work_floats: floats of scratch step_backlog needs for at most B streams of at most T hops (0: none)."""
        return int(self.lib.fe_step_backlog_work_floats(self._h, int(B), int(T)))

    def step_backlog(self, wav_in: Tensor, state: Tensor, wav_out: Optional[Tensor] = None, T: Optional[int] = None, work: Optional[Tensor] = None) -> Tensor:
        """fe_step_backlog: step_chunk for every family - the FastEnhancer models as step_chunk runs them, BSRNN and FSPEN with the T hops
        of each stream on their own time pipeline, LiSenNet as step() walks it.  Arguments, checks and the scratch tensor as for step_chunk,
        with backlog_work_floats(B, T) for the size of work.
        LiSenNet on the time pipeline is opt-in: after set_time_pipeline(P) with P >= 2, a `work` of lisennet_backlog_work_floats(B, T)
        floats is passed through and the chunk (T >= 4) runs pipelined on the caller's state; work=None walks, as at every other setting
        (lisennet_backlog_work(B, T) hands out the engine's scratch tensor at that size, or None where the call would walk anyway)."""
        return self._chunk("fe_step_backlog", "backlog_work_floats", wav_in, state, wav_out, T, work)

    def lisennet_backlog_work_floats(self, B: int, T: int) -> int:
        """fe_lisennet_backlog_work_floats: floats of the work buffer with which step_backlog runs a LiSenNet chunk on the time pipeline
        (counters, windowed frames, the rings of the nine caches); 0 for every other family, for B <= 0 and for T < 4."""
        return int(self.lib.fe_lisennet_backlog_work_floats(self._h, int(B), int(T)))

    def lisennet_backlog_work(self, B: int, T: int) -> Optional[Tensor]:
        """The engine's grow-only scratch tensor at lisennet_backlog_work_floats(B, T) floats for step_backlog(work=...), when the last
        set_time_pipeline() named a width of two or more; else None - the call then walks (what the callers that size the buffer
        themselves pass: streaming.enhance_stream(chunk_hops=...), StreamPool.catch_up)."""
        need = self.lisennet_backlog_work_floats(B, T) if getattr(self, "_time_pipeline", -1) >= 2 else 0
        if need == 0:
            return None
        if getattr(self, "_chunk_work", None) is None or self._chunk_work.numel() < need:
            self._chunk_work = torch.empty(need, dtype=torch.float32, device=self.device)
        return self._chunk_work

    def _chunk(self, entry: str, query: str, wav_in: Tensor, state: Tensor, wav_out: Optional[Tensor], T: Optional[int], work: Optional[Tensor]) -> Tensor:
        """step_chunk / step_backlog: the checks (all of them before any native call), the grow-only scratch tensor, the call of `entry`"""
        H = self.cfg.hop_size
        if not isinstance(wav_in, Tensor) or wav_in.dim() != 2 or wav_in.dtype != torch.float32 or wav_in.stride(1) != 1:
            raise ValueError("wav_in must be a 2-D float32 tensor [B, T*H] with unit stride along the samples")
        B = wav_in.shape[0]
        if T is None:
            T = wav_in.shape[1] // H
        T = operator.index(T)
        if B < 1 or T < 1 or wav_in.shape[1] != T * H:
            raise ValueError(f"wav_in must be [B, T*H] = [B, {T * H}] with B >= 1 and T >= 1, got {tuple(wav_in.shape)}")
        if wav_out is not None and (not isinstance(wav_out, Tensor) or wav_out.dtype != torch.float32 or tuple(wav_out.shape) != (B, T * H)
                                    or wav_out.stride(1) != 1):
            raise ValueError(f"wav_out must be a float32 tensor [{B}, {T * H}] with unit stride along the samples")
        if not isinstance(state, Tensor) or state.dtype != torch.float32 or state.dim() != 1 or not state.is_contiguous():
            raise ValueError("state must be a contiguous 1-D float32 tensor (new_state(B))")
        if work is not None and (not isinstance(work, Tensor) or work.dtype != torch.float32 or not work.is_contiguous()):
            raise ValueError(f"work must be a contiguous float32 tensor of {query}(B, T) floats")
        self._require_gpu()
        if not wav_in.is_cuda or not state.is_cuda or (wav_out is not None and not wav_out.is_cuda) or (work is not None and not work.is_cuda):
            raise ValueError("wav_in, state, wav_out and work must be device tensors")
        if state.numel() != self.state_floats(B):
            raise ValueError(f"state has {state.numel()} floats, a state of {B} streams {self.state_floats(B)}")
        need = getattr(self, query)(B, T)
        if need == 0 and work is not None and entry == "fe_step_backlog":
            need = self.lisennet_backlog_work_floats(B, T)      # (LiSenNet: a work buffer asks for the pipeline, and has to hold its launch)
        if work is None:
            if need > 0:
                if getattr(self, "_chunk_work", None) is None or self._chunk_work.numel() < need:
                    self._chunk_work = torch.empty(need, dtype=torch.float32, device=self.device)
                work = self._chunk_work
        elif work.numel() < need:
            raise ValueError(f"work has {work.numel()} floats, {query}({B}, {T}) = {need}")
        if wav_out is None:
            wav_out = torch.empty(B, T * H, dtype=torch.float32, device=wav_in.device)
        with torch.cuda.device(self.device):
            _lib.check(getattr(self.lib, entry)(self._h, _ptr(wav_in), wav_in.stride(0) if B > 1 else T * H, _ptr(state), _ptr(wav_out),
                                                wav_out.stride(0) if B > 1 else T * H, B, T, _ptr(work), _stream(self.device)), entry)
        return wav_out

    def _slot_tensor(self, slots, capacity: int) -> Tensor:
        """slots -> a device int32 tensor for fe_step_slots / fe_state_reset_slots.  A CUDA int32 tensor is passed through unchecked (the form
        for graph capture: its contents may change from replay to replay); a list or CPU tensor is checked here first - integers in
        [0, capacity), no duplicates - and copied to the device."""
        if isinstance(slots, Tensor) and slots.is_cuda:
            if slots.dtype != torch.int32 or slots.dim() != 1 or not slots.is_contiguous():
                raise ValueError("a device slot tensor must be a contiguous 1-D int32 tensor")
            return slots
        if isinstance(slots, Tensor) and (slots.dim() != 1 or slots.is_floating_point() or slots.is_complex() or slots.dtype == torch.bool):
            raise ValueError("slots must be a 1-D integer tensor")
        vals = []
        for s in (slots.tolist() if isinstance(slots, Tensor) else slots):
            if isinstance(s, bool):
                raise ValueError(f"slot {s!r} is not an integer")
            try:
                vals.append(operator.index(s))
            except TypeError:
                raise ValueError(f"slot {s!r} is not an integer") from None
        for s in vals:
            if not 0 <= s < capacity:
                raise ValueError(f"slot {s} is outside [0, {capacity})")
        if len(set(vals)) != len(vals):
            raise ValueError("duplicate slots")
        if not 1 <= len(vals) <= capacity:
            raise ValueError(f"{len(vals)} slots for a capacity of {capacity}")
        self._require_gpu()
        return torch.tensor(vals, dtype=torch.int32).to(self.device, non_blocking=False)

    def step_slots(self, wav_in: Tensor, state: Tensor, capacity: int, slots, wav_out: Optional[Tensor] = None, T: int = 1) -> Tensor:
        """fe_step_slots: wav_in [n, T*H] (row i = state slot slots[i]) -> wav_out [n, T*H]; only the named slots of `state`
        (sized for `capacity` streams) are updated.  slots: a list / CPU tensor (checked) or a CUDA int32 tensor (not checked)."""
        return self._step(wav_in, state, wav_out, T, capacity, slots)

    def step_pool(self, wav_in: Tensor, state: Tensor, capacity: int, slots, wav_out: Optional[Tensor] = None, T: int = 1) -> Tensor:
        """fe_step_pool: step_slots for every family with a streaming state - FastEnhancer's models as step_slots runs them, BSRNN, FSPEN and
        LiSenNet on the slotted forms of their per-stream kernels.  Arguments and checks as for step_slots."""
        return self._step(wav_in, state, wav_out, T, capacity, slots, pool=True)

    def reset_slots(self, state: Tensor, capacity: int, slots) -> None:
        """fe_state_reset_slots: the named slots of `state` (sized for `capacity` streams) as fe_state_init leaves them (zero)."""
        sl = self._slot_tensor(slots, capacity)
        self._require_gpu()
        assert state.numel() == self.state_floats(capacity) and state.is_contiguous()
        with torch.cuda.device(self.device):
            _lib.check(self.lib.fe_state_reset_slots(self._h, _ptr(state), int(capacity), _ptr(sl), sl.numel(), _stream(self.device)),
                       "fe_state_reset_slots")
        self._slots_keep = sl

    # ---- state records: a stream's state as a capacity-1 state buffer (fe_state_export_slots / fe_state_import_slots)
    @property
    def record_floats(self) -> int:
        """floats of one stream's state record: state_floats(1)"""
        return self.state_floats(1)

    def _records(self, records: Tensor, n: int) -> Tensor:
        """records -> float32 [n, record_floats], rows back to back, on this engine's device or in page-locked host memory (any 4-byte
        alignment: a view into a larger buffer is fine).  Anything else is a ValueError before any native call."""
        rf = self.record_floats
        if not isinstance(records, Tensor) or records.dtype != torch.float32 or tuple(records.shape) != (n, rf):
            raise ValueError(f"records must be a float32 tensor [{n}, {rf}], got {getattr(records, 'dtype', type(records).__name__)} "
                             f"{tuple(getattr(records, 'shape', ()))}")
        if records.stride(1) != 1 or (n > 1 and records.stride(0) != rf):
            raise ValueError("records must lie back to back (row stride = record_floats, unit stride inside a record)")
        if records.is_cuda:
            if records.device != self.device:
                raise ValueError(f"records are on {records.device}, the engine on {self.device}: carry them through page-locked host memory")
        elif not records.is_pinned():
            raise ValueError("host records must be in page-locked memory: pin the buffer (pin_memory())")
        return records

    def _move_records(self, name: str, state: Tensor, capacity: int, slots, records: Optional[Tensor]) -> Tensor:
        if records is not None:       # (before the slots: a list of them is copied to the device by its check)
            records = self._records(records, slots.numel() if isinstance(slots, Tensor) else len(slots))
        sl = self._slot_tensor(slots, capacity)
        n = sl.numel()
        self._require_gpu()
        assert state.is_cuda and state.numel() == self.state_floats(capacity) and state.is_contiguous()
        if records is None:
            records = torch.empty(n, self.record_floats, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(getattr(self.lib, name)(self._h, _ptr(state), int(capacity), _ptr(sl), _ptr(records), n, _stream(self.device)), name)
        self._slots_keep = sl            # (alive until the next call - the launch is asynchronous)
        if not records.is_cuda:
            self._pinned_keep = (records,)
        return records

    def export_slots(self, state: Tensor, capacity: int, slots, out: Optional[Tensor] = None) -> Tensor:
        """fe_state_export_slots: the state records [n, record_floats] of the named slots of `state` (sized for `capacity` streams), which is
        not written.  out: a CUDA tensor of this device or a page-locked CPU tensor (a new CUDA tensor when None).  slots as for step_slots;
        a slot out of range (device slot tensors only) yields a fresh stream's record.  Asynchronous on the current stream: synchronise it
        before reading host records."""
        return self._move_records("fe_state_export_slots", state, capacity, slots, out)

    def import_slots(self, state: Tensor, capacity: int, slots, records: Tensor) -> None:
        """fe_state_import_slots: slot slots[i] of `state` becomes records[i] (device or page-locked host memory); no other float of the
        state is written.  Asynchronous on the current stream: host records must stay as they are until it has completed."""
        if records is None:
            raise ValueError("records must be a float32 tensor")
        self._move_records("fe_state_import_slots", state, capacity, slots, records)

    def _pinned_audio(self, name: str, x: Optional[Tensor], rows: int, T: int) -> Tensor:
        """x -> a page-locked CPU float32 tensor [rows, T*H] (row stride free), or a fresh one when x is None.  Anything else is a
        ValueError before any native call: the kernel reads and writes this memory over PCIe, and unpinned memory would fault it."""
        H = self.cfg.hop_size
        if x is None:
            return torch.empty(rows, T * H, dtype=torch.float32).pin_memory()
        if not isinstance(x, Tensor) or x.device.type != "cpu":
            raise ValueError(f"{name} must be a CPU tensor in page-locked memory (pin_memory()), not {getattr(x, 'device', type(x).__name__)}")
        if not x.is_pinned():
            raise ValueError(f"{name} is not in page-locked memory: pin the buffer (pin_memory())")
        if x.dtype != torch.float32 or x.dim() != 2 or x.stride(1) != 1 or tuple(x.shape) != (rows, T * H):
            raise ValueError(f"{name} must be float32 [{rows}, {T * H}] with unit stride along the samples, got {x.dtype} {tuple(x.shape)}")
        return x

    def step_pinned(self, wav_in: Tensor, state: Tensor, wav_out: Optional[Tensor] = None, T: int = 1) -> Tensor:
        """fe_step_pinned: wav_in [B, T*H] in page-locked HOST memory -> wav_out [B, T*H] in page-locked host memory (allocated when None),
        one launch that reads and writes the audio over PCIe; state (device) updated in place.  Asynchronous on the current stream:
        synchronise it before reading wav_out or rewriting wav_in."""
        return self._step(wav_in, state, wav_out, T, pinned=True)

    def step_slots_pinned(self, wav_in: Tensor, state: Tensor, capacity: int, slots, wav_out: Optional[Tensor] = None, T: int = 1) -> Tensor:
        """fe_step_slots_pinned: step_slots with wav_in / wav_out [n, T*H] in page-locked HOST memory (wav_out allocated when None).
        slots as for step_slots.  Asynchronous on the current stream: synchronise it before reading wav_out or rewriting wav_in."""
        return self._step(wav_in, state, wav_out, T, capacity, slots, pinned=True)

    # ---- packet audio: per-stream hop counts and offsets, float32 or int16 PCM (fe_step_streams / fe_step_streams_pinned)
    @staticmethod
    def pack_stream_desc(desc) -> Tensor:
        """[(slot, hops, in_offset, out_offset), ...] -> a CPU int32 tensor [n, 6], the memory image of n fe_stream_desc."""
        rows = [tuple(operator.index(v) for v in d) for d in desc]
        if any(len(r) != 4 for r in rows):
            raise ValueError("a stream descriptor is (slot, hops, in_offset, out_offset)")
        arr = (_lib.fe_stream_desc * max(len(rows), 1))(*[_lib.fe_stream_desc(*r) for r in rows])
        words = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.int32).view(-1, 6)
        return words[:len(rows)].clone()

    def _stream_desc_tensor(self, desc, capacity: int, T_max: int, in_count: int, out_count: int) -> Tensor:
        """desc -> a device int32 tensor [n, 6].  A CUDA int32 tensor [n, 6] is passed through unchecked (the form for graph capture: the
        kernel checks every descriptor itself); a list of (slot, hops, in_offset, out_offset) is checked here first - slots in [0, capacity)
        without duplicates, 0 <= hops <= T_max, both ranges inside their buffers - and copied to the device."""
        H = self.cfg.hop_size
        if isinstance(desc, Tensor):
            if desc.dtype != torch.int32 or desc.dim() != 2 or desc.shape[1] != 6 or not desc.is_contiguous():
                raise ValueError("a descriptor tensor must be a contiguous int32 tensor [n, 6] (Engine.pack_stream_desc)")
            if desc.is_cuda:
                return desc
            self._require_gpu()
            return desc.to(self.device)
        rows = [tuple(operator.index(v) for v in d) for d in desc]
        if not 1 <= len(rows) <= capacity:
            raise ValueError(f"{len(rows)} streams for a capacity of {capacity}")
        for slot, hops, i0, o0 in rows:
            if not 0 <= slot < capacity:
                raise ValueError(f"slot {slot} is outside [0, {capacity})")
            if not 0 <= hops <= T_max:
                raise ValueError(f"hops {hops} is outside [0, {T_max}]")
            if i0 < 0 or i0 + hops * H > in_count:
                raise ValueError(f"slot {slot}: input range [{i0}, {i0 + hops * H}) is outside [0, {in_count})")
            if o0 < 0 or o0 + hops * H > out_count:
                raise ValueError(f"slot {slot}: output range [{o0}, {o0 + hops * H}) is outside [0, {out_count})")
        if len({r[0] for r in rows}) != len(rows):
            raise ValueError("duplicate slots")
        self._require_gpu()
        return self.pack_stream_desc(rows).to(self.device)

    @staticmethod
    def _stream_table(what: str, t: Optional[Tensor], shape) -> Optional[Tensor]:
        """min_gain [capacity] / levels [capacity, 4] of the ctl steps: float32, contiguous, on the device or in page-locked host memory"""
        if t is None:
            return None
        if not isinstance(t, Tensor) or t.dtype != torch.float32 or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
            raise ValueError(f"{what} must be a contiguous float32 tensor {list(shape)}")
        if not t.is_cuda and not (t.device.type == "cpu" and t.is_pinned()):
            raise ValueError(f"{what} must be a device tensor or a CPU tensor in page-locked memory (pin_memory())")
        return t

    @staticmethod
    def _bank_table(t: Optional[Tensor], capacity: int) -> Optional[Tensor]:
        """bank [capacity] of the banked steps: int32, contiguous, on the device or in page-locked host memory"""
        if t is None:
            return None
        if not isinstance(t, Tensor) or t.dtype != torch.int32 or tuple(t.shape) != (capacity,) or not t.is_contiguous():
            raise ValueError(f"bank must be a contiguous int32 tensor [{capacity}]")
        if not t.is_cuda and not (t.device.type == "cpu" and t.is_pinned()):
            raise ValueError("bank must be a device tensor or a CPU tensor in page-locked memory (pin_memory())")
        return t

    def _step_streams(self, wav_in: Tensor, state: Tensor, capacity: int, desc, wav_out: Tensor, T_max: int, pinned: bool,
                      min_gain: Optional[Tensor] = None, levels: Optional[Tensor] = None, bank: Optional[Tensor] = None, chunk: bool = False,
                      work: Optional[Tensor] = None, pool: bool = False, pool_ctl: bool = False, pool_chunk: bool = False) -> Tensor:
        """The packet step behind step_streams* / step_streams_chunk* / step_pool_streams*.  pool: fe_step_pool_streams[_pinned], the packet
        step of every family - the same checks of buffers and descriptors; the per-stream controls, the weight banks and the pipelined form
        are FastEnhancer's and are refused here.  pool_ctl: fe_step_pool_streams_ctl[_pinned], that step with the two controls for every
        family (either table may be None: a NULL).  pool_chunk: fe_step_pool_streams_chunk[_pinned], the pipelined form of pool_ctl - the
        checks and the scratch of chunk, no bank table."""
        ctl = min_gain is not None or levels is not None or pool_ctl
        chunk = chunk or pool_chunk
        name = "fe_step_streams" + ("_banked" if bank is not None else "_ctl" if ctl else "") + ("_pinned" if pinned else "")
        if chunk:       # (one entry point, every table an argument that may be NULL)
            name = "fe_step_streams_chunk" + ("_pinned" if pinned else "")
        if pool:
            given = [k for k, v in (("min_gain", min_gain), ("levels", levels), ("bank", bank), ("chunk", chunk or None)) if v is not None]
            if given:
                raise ValueError(f"step_pool_streams takes no {' / '.join(given)}: the suppression limit, the level meters, the weight banks and the "
                                 "pipelined packet step are built for the FastEnhancer family (step_streams, step_streams_chunk)")
            name = "fe_step_pool_streams" + ("_pinned" if pinned else "")
        if pool_ctl:
            name = "fe_step_pool_streams_ctl" + ("_pinned" if pinned else "")
        if pool_chunk:
            name = "fe_step_pool_streams_chunk" + ("_pinned" if pinned else "")
        work_query = self.pool_streams_chunk_work_floats if pool_chunk else self.streams_chunk_work_floats
        # (LiSenNet pipelines this call on request: after set_time_pipeline(P >= 2) the scratch is that launch's - the rule of lisennet_backlog_work)
        on_request = pool_chunk and packet_chunk_on_request(self)
        if on_request:
            work_query = self.lisennet_pool_streams_chunk_work_floats
        for what, x in (("wav_in", wav_in), ("wav_out", wav_out)):
            if not isinstance(x, Tensor) or x.dtype not in (torch.float32, torch.int16) or not x.is_contiguous() or x.numel() == 0:
                raise ValueError(f"{what} must be a contiguous, non-empty float32 or int16 tensor")
        if wav_in.dtype != wav_out.dtype:
            raise ValueError(f"wav_in is {wav_in.dtype} and wav_out {wav_out.dtype}: one format per call")
        for what, x in (("wav_in", wav_in), ("wav_out", wav_out)):
            if pinned and (x.device.type != "cpu" or not x.is_pinned()):
                raise ValueError(f"{what} must be a CPU tensor in page-locked memory (pin_memory())")
            if not pinned and not x.is_cuda:
                raise ValueError(f"{what} must be a device tensor ({name}_pinned takes page-locked host memory)")
        if T_max < 1:
            raise ValueError("T_max must be at least 1")
        min_gain = self._stream_table("min_gain", min_gain, (capacity,))
        levels = self._stream_table("levels", levels, (capacity, 4))
        bank = self._bank_table(bank, capacity)
        if chunk and work is not None:
            if not isinstance(work, Tensor) or work.dtype != torch.float32 or not work.is_contiguous():
                raise ValueError(f"work must be a contiguous float32 tensor of {work_query.__name__}(n, T_max) floats")
            # (the windowed frames [n][T_max][N] at least, where the model pipelines at all: known without the library)
            n_desc = desc.shape[0] if isinstance(desc, Tensor) else len(desc)
            c = self.cfg      # (the default, ln and dprnn models: the ring variants, the noncausal model and the baselines never pipeline this call)
            pipelines = hasattr(c, "rf_blocks") and not getattr(c, "dpt", False) and getattr(c, "kernel_size_time", 1) == 1 and not getattr(c, "noncausal", False)
            if pool_chunk and self.family.pool:       # (the pool call: the families whose time pipeline carries the streaming state - BSRNN, FSPEN)
                pipelines = self.family.backlog or on_request
            if T_max >= 4 and pipelines and work.numel() < n_desc * T_max * c.n_fft:
                raise ValueError(f"work has {work.numel()} floats, {n_desc} streams of up to {T_max} hops need at least {n_desc * T_max * self.cfg.n_fft} "
                                 f"({work_query.__name__})")
        d = self._stream_desc_tensor(desc, capacity, T_max, wav_in.numel(), wav_out.numel())
        self._require_gpu()
        assert state.is_cuda and state.numel() == self.state_floats(capacity) and state.is_contiguous()
        fmt = _lib.FE_AUDIO_S16 if wav_in.dtype == torch.int16 else _lib.FE_AUDIO_F32
        tables = (_ptr(min_gain), _ptr(levels), _ptr(bank)) if bank is not None else (_ptr(min_gain), _ptr(levels)) if ctl else ()
        if chunk:
            need = work_query(d.shape[0], T_max)
            if work is None:
                if need > 0:        # (a scratch tensor kept on the engine, grown when needed; pass `work` inside a graph capture)
                    if getattr(self, "_streams_chunk_work", None) is None or self._streams_chunk_work.numel() < need:
                        self._streams_chunk_work = torch.empty(need, dtype=torch.float32, device=self.device)
                    work = self._streams_chunk_work
            elif not work.is_cuda:
                raise ValueError("work must be a device tensor")
            elif work.numel() < need:
                raise ValueError(f"work has {work.numel()} floats, {work_query.__name__}({d.shape[0]}, {T_max}) is {need}")
            tables = (_ptr(min_gain), _ptr(levels), _ptr(work)) if pool_chunk else (_ptr(min_gain), _ptr(levels), _ptr(bank), _ptr(work))
        with torch.cuda.device(self.device):
            _lib.check(getattr(self.lib, name)(self._h, _ptr(wav_in), wav_in.numel(), _ptr(state), int(capacity), _ptr(d), _ptr(wav_out), wav_out.numel(),
                                               d.shape[0], int(T_max), fmt, *tables, _stream(self.device)), name)
        self._desc_keep = (d, min_gain, levels, bank, work)    # (alive until the next call - the launch is asynchronous)
        if pinned:
            self._pinned_keep = (wav_in, wav_out)
        return wav_out

    def step_streams(self, wav_in: Tensor, state: Tensor, capacity: int, desc, wav_out: Tensor, T_max: int = 1, *,
                     min_gain: Optional[Tensor] = None, levels: Optional[Tensor] = None, bank: Optional[Tensor] = None) -> Tensor:
        """fe_step_streams: every stream of `desc` advances its own number of hops (0 .. T_max), reading wav_in [in_offset + t*H ...] and
        writing wav_out [out_offset + t*H ...] - flat device buffers, both float32 or both int16 PCM (full scale 32768).  desc: a list of
        (slot, hops, in_offset, out_offset) (checked) or a CUDA int32 tensor [n, 6] (pack_stream_desc; checked by the kernel only).
        min_gain / levels (fe_step_streams_ctl, when either is given): float32 tables indexed by SLOT, on the device or in page-locked host
        memory, read and written by the kernel when it runs.  min_gain [capacity]: the least net amplitude gain of a bin, linear in [0, 1]
        (0 = no limit).  levels [capacity, 4]: (in_sumsq, in_peak, out_sumsq, out_peak) of every stream that advanced at least one hop.
        bank (fe_step_streams_banked, when given): an int32 table [capacity] indexed by SLOT, device or page-locked host memory, read by the
        kernel when it runs: the weight bank (set_weight_banks, load_state_dict(bank=)) the stream of that slot runs on; every bank of the
        engine must be loaded; a bank out of range makes the stream one without state (zero rows)."""
        return self._step_streams(wav_in, state, capacity, desc, wav_out, T_max, pinned=False, min_gain=min_gain, levels=levels, bank=bank)

    def step_streams_pinned(self, wav_in: Tensor, state: Tensor, capacity: int, desc, wav_out: Tensor, T_max: int = 1, *,
                            min_gain: Optional[Tensor] = None, levels: Optional[Tensor] = None, bank: Optional[Tensor] = None) -> Tensor:
        """fe_step_streams_pinned: step_streams with wav_in / wav_out in page-locked HOST memory, read and written by the kernel over PCIe.
        Asynchronous on the current stream: synchronise it before reading wav_out (or a pinned levels table) or rewriting wav_in."""
        return self._step_streams(wav_in, state, capacity, desc, wav_out, T_max, pinned=True, min_gain=min_gain, levels=levels, bank=bank)

    def step_pool_streams(self, wav_in: Tensor, state: Tensor, capacity: int, desc, wav_out: Tensor, T_max: int = 1, *,
                          min_gain=None, levels=None, bank=None, chunk=None) -> Tensor:
        """fe_step_pool_streams: step_streams for every family with a streaming state - FastEnhancer's models as step_streams runs them,
        BSRNN, FSPEN and LiSenNet on the packet forms of their per-stream kernels (what step_pool(T = T_max) launches; allocates nothing:
        init_state sizes the scratch of BSRNN's three-launch step).  Buffers, descriptors and their checks as for step_streams; wav_in and
        wav_out must not overlap.  min_gain, levels, bank and chunk are FastEnhancer's (step_streams, step_streams_chunk): a ValueError here."""
        return self._step_streams(wav_in, state, capacity, desc, wav_out, T_max, pinned=False, min_gain=min_gain, levels=levels, bank=bank,
                                  chunk=chunk, pool=True)

    def step_pool_streams_pinned(self, wav_in: Tensor, state: Tensor, capacity: int, desc, wav_out: Tensor, T_max: int = 1, *,
                                 min_gain=None, levels=None, bank=None, chunk=None) -> Tensor:
        """fe_step_pool_streams_pinned: step_pool_streams with wav_in / wav_out in page-locked HOST memory (the completion rule of
        step_streams_pinned: synchronise the stream before reading wav_out or rewriting wav_in)."""
        return self._step_streams(wav_in, state, capacity, desc, wav_out, T_max, pinned=True, min_gain=min_gain, levels=levels, bank=bank,
                                  chunk=chunk, pool=True)

    def step_pool_streams_ctl(self, wav_in: Tensor, state: Tensor, capacity: int, desc, wav_out: Tensor, T_max: int = 1, *,
                              min_gain: Optional[Tensor] = None, levels: Optional[Tensor] = None) -> Tensor:
        """fe_step_pool_streams_ctl: step_pool_streams with the suppression limit and the level meters for every family with a streaming state -
        FastEnhancer's models as step_streams(min_gain=, levels=) runs them; BSRNN, FSPEN and LiSenNet inside the launches of step_pool_streams.
        min_gain [capacity] / levels [capacity, 4]: the tables of step_streams, with its checks (float32, contiguous, indexed by SLOT, on the
        device or in page-locked host memory); either may be None, both None is step_pool_streams.  On BSRNN, FSPEN and LiSenNet the limit
        holds the output bin against the input bin, |Y| >= min_gain |X| (their outputs are not a mask times the input); every state tensor
        but cache_istft keeps the bits of the unlimited run."""
        return self._step_streams(wav_in, state, capacity, desc, wav_out, T_max, pinned=False, min_gain=min_gain, levels=levels, pool_ctl=True)

    def step_pool_streams_ctl_pinned(self, wav_in: Tensor, state: Tensor, capacity: int, desc, wav_out: Tensor, T_max: int = 1, *,
                                     min_gain: Optional[Tensor] = None, levels: Optional[Tensor] = None) -> Tensor:
        """fe_step_pool_streams_ctl_pinned: step_pool_streams_ctl with wav_in / wav_out in page-locked HOST memory (the completion rule of
        step_streams_pinned: synchronise the stream before reading wav_out or a pinned levels table, or rewriting wav_in)."""
        return self._step_streams(wav_in, state, capacity, desc, wav_out, T_max, pinned=True, min_gain=min_gain, levels=levels, pool_ctl=True)

    # ---- the packet step on the time pipeline: streams that come back with a backlog (fe_step_streams_chunk[_pinned])
    def streams_chunk_work_floats(self, n: int, T_max: int) -> int:
        """fe_step_streams_chunk_work_floats: floats of scratch step_streams_chunk needs for at most n streams of at most T_max hops (0: none)."""
        return int(self.lib.fe_step_streams_chunk_work_floats(self._h, int(n), int(T_max)))

    def step_streams_chunk(self, wav_in: Tensor, state: Tensor, capacity: int, desc, wav_out: Tensor, T_max: int, *,
                           min_gain: Optional[Tensor] = None, levels: Optional[Tensor] = None, bank: Optional[Tensor] = None,
                           work: Optional[Tensor] = None) -> Tensor:
        """fe_step_streams_chunk: step_streams(..., min_gain=, levels=, bank=) with the hops of EACH stream spread over the time pipeline - the
        same descriptors, slots, formats, limit, meters and banks, in place on the capacity-sized state.  Results agree with step_streams to
        fp32 rounding (cache_stft bit for bit); wav_in and wav_out must not overlap.  Where nothing is pipelined (T_max < 4, more than
        #CUs / 2 streams, set_time_pipeline(0 | 1), the time_kernel / dptransformer models) the call is step_streams itself, bit for bit
        (last_step_kernel() says which ran).  work: a float32 device tensor of at least streams_chunk_work_floats(n, T_max) floats (the form
        for graph capture); None: a scratch tensor kept on the engine, grown when needed."""
        return self._step_streams(wav_in, state, capacity, desc, wav_out, T_max, pinned=False, min_gain=min_gain, levels=levels, bank=bank,
                                  chunk=True, work=work)

    def step_streams_chunk_pinned(self, wav_in: Tensor, state: Tensor, capacity: int, desc, wav_out: Tensor, T_max: int, *,
                                  min_gain: Optional[Tensor] = None, levels: Optional[Tensor] = None, bank: Optional[Tensor] = None,
                                  work: Optional[Tensor] = None) -> Tensor:
        """fe_step_streams_chunk_pinned: step_streams_chunk with wav_in / wav_out in page-locked HOST memory (the completion rule of
        step_streams_pinned: synchronise the stream before reading wav_out or rewriting wav_in)."""
        return self._step_streams(wav_in, state, capacity, desc, wav_out, T_max, pinned=True, min_gain=min_gain, levels=levels, bank=bank,
                                  chunk=True, work=work)

    # ---- ... for every family with a streaming state (fe_step_pool_streams_chunk[_pinned])
    def pool_streams_chunk_work_floats(self, n: int, T_max: int) -> int:
        """fe_step_pool_streams_chunk_work_floats: floats of scratch step_pool_streams_chunk needs for at most n streams of at most T_max
        hops (0: none - T_max < 4, LiSenNet, the FastEnhancer models whose streams_chunk_work_floats is 0)."""
        return int(self.lib.fe_step_pool_streams_chunk_work_floats(self._h, int(n), int(T_max)))

    def lisennet_pool_streams_chunk_work_floats(self, n: int, T_max: int) -> int:
        """fe_lisennet_pool_streams_chunk_work_floats: floats of the work buffer with which step_pool_streams_chunk runs a LiSenNet packet
        call on the time pipeline (counters, windowed frames, the rings of the nine caches), whatever set_time_pipeline says at the time of
        the query; 0 for every other family, for n <= 0 and for T_max < 4."""
        return int(self.lib.fe_lisennet_pool_streams_chunk_work_floats(self._h, int(n), int(T_max)))

    def step_pool_streams_chunk(self, wav_in: Tensor, state: Tensor, capacity: int, desc, wav_out: Tensor, T_max: int, *,
                                min_gain: Optional[Tensor] = None, levels: Optional[Tensor] = None, work: Optional[Tensor] = None) -> Tensor:
        """fe_step_pool_streams_chunk: step_pool_streams_ctl(..., min_gain=, levels=) with the hops of EACH stream spread over the time
        pipeline - the same descriptors, slots, formats, limit and meters, in place on the capacity-sized state.  FastEnhancer's models as
        step_streams_chunk runs them; BSRNN and FSPEN on the time-pipelined packet form of their frame kernels, results agreeing with
        step_pool_streams_ctl to fp32 rounding (cache_stft bit for bit); every call that is not pipelined (T_max < 4,
        set_time_pipeline(0 | 1), too many streams) as step_pool_streams_ctl itself, bit for bit (last_step_kernel() says which ran).
        wav_in and wav_out must not overlap.  work: a float32 device tensor of at least pool_streams_chunk_work_floats(n, T_max) floats
        (the form for graph capture); None: a scratch tensor kept on the engine, grown when needed.
        LiSenNet on the time pipeline is opt-in: after set_time_pipeline(P) with P >= 2 the call runs the time-pipelined packet form of
        its frame kernel on the slots' nine caches in place, with a `work` of lisennet_pool_streams_chunk_work_floats(n, T_max) floats
        (checked; None: the engine's scratch tensor at that size).  At every other setting it is step_pool_streams_ctl itself,
        pool_streams_chunk_work_floats is 0 and a `work` is passed through unread."""
        return self._step_streams(wav_in, state, capacity, desc, wav_out, T_max, pinned=False, min_gain=min_gain, levels=levels, work=work,
                                  pool_chunk=True)

    def step_pool_streams_chunk_pinned(self, wav_in: Tensor, state: Tensor, capacity: int, desc, wav_out: Tensor, T_max: int, *,
                                       min_gain: Optional[Tensor] = None, levels: Optional[Tensor] = None, work: Optional[Tensor] = None) -> Tensor:
        """fe_step_pool_streams_chunk_pinned: step_pool_streams_chunk with wav_in / wav_out in page-locked HOST memory (the completion rule
        of step_streams_pinned: synchronise the stream before reading wav_out or a pinned levels table, or rewriting wav_in)."""
        return self._step_streams(wav_in, state, capacity, desc, wav_out, T_max, pinned=True, min_gain=min_gain, levels=levels, work=work,
                                  pool_chunk=True)

    def new_pinned(self, *shape: int, dtype=torch.float32) -> Tensor:
        """a zeroed page-locked host tensor (the audio of the pinned steps)"""
        self._require_gpu()
        return torch.zeros(*shape, dtype=dtype).pin_memory()

    def synchronize(self) -> None:
        """wait for the current stream of the engine's device (the completion rule of the pinned steps)"""
        self._require_gpu()
        torch.cuda.current_stream(self.device).synchronize()

    def step_host(self, wav_in: Tensor, state: Tensor, wav_out: Optional[Tensor] = None, T: int = 1) -> Tensor:
        """fe_step_host: wav_in [B, n*T*H] in HOST memory (pinned for full speed) -> wav_out [B, n*T*H] in host memory, n calls of T hops
        each with the copies of the neighbouring calls under each kernel; state (device) updated in place.  Asynchronous on the current
        stream: synchronise it before reading wav_out."""
        self._require_gpu()
        B, H = wav_in.shape[0], self.cfg.hop_size
        assert not wav_in.is_cuda and wav_in.dtype == torch.float32 and wav_in.stride(1) == 1 and wav_in.shape[1] % (T * H) == 0
        assert state.numel() == self.state_floats(B) and state.is_contiguous() and state.is_cuda
        n = wav_in.shape[1] // (T * H)
        if wav_out is None:
            wav_out = torch.empty(B, n * T * H, dtype=torch.float32).pin_memory()
        assert not wav_out.is_cuda and wav_out.stride(1) == 1 and wav_out.shape == wav_in.shape
        work = torch.empty(4 * B * T * H, dtype=torch.float32, device=self.device)
        self._host_work = work          # (kept until the next call: the launches are asynchronous)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.fe_step_host(self._h, ctypes.c_void_p(wav_in.data_ptr()), wav_in.stride(0) if B > 1 else n * T * H, _ptr(state),
                                             ctypes.c_void_p(wav_out.data_ptr()), wav_out.stride(0) if B > 1 else n * T * H, B, T, n, _ptr(work),
                                             _stream(self.device)), "fe_step_host")
        return wav_out

    def set_step_kernel(self, kernel: str):
        """fe_set_step_kernel: "waves4" (the 256-thread kernel) | "wg8" (default: the 512-thread per-hop kernel where built) | "wg8_persist"."""
        code = {"waves4": _lib.FE_STEP_KERNEL_WAVES4, "wg8": _lib.FE_STEP_KERNEL_WG8, "wg8_persist": _lib.FE_STEP_KERNEL_WG8_PERSIST}[kernel]
        _lib.check(self.lib.fe_set_step_kernel(self._h, code), "fe_set_step_kernel")

    def set_option(self, name: str, value: int):
        """fe_set_option: the other kernel-selection switches of the handle by name ("bsrnn_role_split", "bsrnn_stream_batch_min",
        "bsrnn_three_launch_step", "bsrnn_ov_profile", "fspen_stream_batch_min", "low_lds_companion", "bsrnn_fused_step", "lisennet_stream_batch_min";
        include/fastenhancer_hip.h)."""
        _lib.check(self.lib.fe_set_option(self._h, name.encode(), int(value)), "fe_set_option")

    def get_option(self, name: str) -> int:
        v = ctypes.c_int(0)
        _lib.check(self.lib.fe_get_option(self._h, name.encode(), ctypes.byref(v)), "fe_get_option")
        return v.value

    def option_names(self):
        return [self.lib.fe_option_name(i).decode() for i in range(self.lib.fe_options())]

    def last_step_kernel(self) -> str:
        """fe_last_step_kernel: what the last compute call of this handle enqueued (kernel families / instantiations + the compiled shape)."""
        return self.lib.fe_last_step_kernel(self._h).decode()

    def set_offline_engine(self, engine: str):
        """fe_set_offline_engine: "auto" | "frame_walk" | "time_batched" (the layer-by-layer engine of csrc/tb_kernels.hip.h)"""
        code = {"auto": _lib.FE_OFFLINE_AUTO, "frame_walk": _lib.FE_OFFLINE_FRAME_WALK, "time_batched": _lib.FE_OFFLINE_TIME_BATCHED}[engine]
        _lib.check(self.lib.fe_set_offline_engine(self._h, code), "fe_set_offline_engine")

    def set_time_pipeline(self, frames_in_flight: int):
        """fe_set_time_pipeline: workgroups per stream in offline / spec launches with T >= 4 (0 = one workgroup per stream)."""
        _lib.check(self.lib.fe_set_time_pipeline(self._h, int(frames_in_flight)), "fe_set_time_pipeline")
        self._time_pipeline = int(frames_in_flight)       # (lisennet_backlog_work: an explicit width >= 2 opts LiSenNet's backlogs in)

    def model_state_floats(self, B: int) -> int:
        """floats of the model's own caches (fe_spec_step's h_dev): the state without the two STFT caches"""
        return self.state_floats(B) - 2 * B * self.cfg.cache_len

    def spec_step(self, spec: Tensor, h: Tensor) -> Tensor:
        """spec [B, N/2+1, T, 2], h = the model caches in C ABI order (K x [B*F2, C2]; time_kernel: + the conv caches),
        updated in place -> spec_hat [B, N/2+1, T, 2]."""
        self._require_gpu()
        B, Fb, T, two = spec.shape
        assert Fb == self.cfg.F0 + 1 and two == 2 and spec.is_contiguous() and h.is_contiguous()
        assert h.numel() == self.model_state_floats(B), (h.numel(), self.model_state_floats(B))
        out = torch.empty_like(spec)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.fe_spec_step(self._h, _ptr(spec), _ptr(h), _ptr(out), B, T, _stream(self.device)), "fe_spec_step")
        return out

    def offline(self, noisy: Tensor) -> Tuple[Tensor, Tensor]:
        """Model.forward (model.py:728-735): noisy [B, Tw] -> (wav_hat [B, H*(Tw//H)], spec_hat [B, N/2, T, 2])."""
        self._require_gpu()
        if noisy.dim() == 3:            # [B, 1, Tw] -> [B, Tw]  (functional/audio_modules.py:73-74)
            noisy = noisy.squeeze(1)
        noisy = noisy.contiguous().float()
        B, Tw = noisy.shape
        cfg = self.cfg
        T = 1 + Tw // cfg.hop_size
        wav = torch.empty(B, cfg.hop_size * (T - 1), dtype=torch.float32, device=noisy.device)
        spec = torch.empty(B, self.family.spec_bins(cfg), T, 2, dtype=torch.float32, device=noisy.device)
        work = torch.empty(int(self.lib.fe_offline_work_floats(self._h, B, Tw)), dtype=torch.float32, device=noisy.device)
        self._last_work = work          # (tools/gpu_tb_check.py looks at the time-batched engine's intermediate buffers)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.fe_offline(self._h, _ptr(noisy), B, Tw, _ptr(wav), _ptr(spec), _ptr(work), _stream(self.device)),
                       "fe_offline")
        return wav, spec

    def offline_ragged(self, noisy: List[Tensor]) -> Tuple[List[Tensor], List[Tensor]]:
        """Model.forward over utterances of different lengths in ONE call (fe_offline_ragged; the reference enhances a directory file by
        file, scripts/test_pytorch.py:28-37): noisy = B tensors [Tw_b] (or [1, Tw_b]) -> (B wavs [H * (Tw_b // H)], B specs [F, T_b, 2])."""
        self._require_gpu()
        cfg, dev = self.cfg, self.device
        xs = [t.reshape(-1).to(dev, torch.float32) for t in noisy]
        B = len(xs)
        lens = [int(t.numel()) for t in xs]
        Tw = max(lens)
        Tmax = 1 + Tw // cfg.hop_size
        F = self.family.spec_bins(cfg)
        batch = torch.zeros(B, Tw, dtype=torch.float32, device=dev)
        for b, t in enumerate(xs):
            batch[b, :lens[b]] = t
        n_out = cfg.hop_size * (Tmax - 1)
        wav = torch.zeros(B, n_out, dtype=torch.float32, device=dev)
        spec = torch.empty(B, F, Tmax, 2, dtype=torch.float32, device=dev)
        work = torch.empty(int(self.lib.fe_offline_ragged_work_floats(self._h, B, Tw)), dtype=torch.float32, device=dev)
        self._last_work = work
        lens_c = (ctypes.c_int * B)(*lens)
        with torch.cuda.device(dev):
            _lib.check(self.lib.fe_offline_ragged(self._h, _ptr(batch), Tw, lens_c, B, _ptr(wav), n_out, _ptr(spec), _ptr(work), _stream(dev)),
                       "fe_offline_ragged")
        Tb = [1 + n // cfg.hop_size for n in lens]
        return [wav[b, :cfg.hop_size * (Tb[b] - 1)] for b in range(B)], [spec[b, :, :Tb[b]] for b in range(B)]

    # ------------------------------------------------------------------ stand-alone STFT / iSTFT (the `.stft` modules)
    def stft_step(self, wav_in: Tensor, cache: Tensor) -> Tuple[Tensor, Tensor]:
        """ONNXSTFT.forward: wav_in [B, H], cache [B, N-H] -> (spec [B, N/2+1, 1, 2], cache'); inputs untouched."""
        self._require_gpu()
        B, c = wav_in.shape[0], self.cfg
        wav_in = wav_in.to(self.device, torch.float32)
        cache = cache.to(self.device, torch.float32).contiguous()
        assert wav_in.shape[1] == c.hop_size and wav_in.stride(1) == 1 and tuple(cache.shape) == (B, c.cache_len)
        spec = torch.empty(B, c.n_fft // 2 + 1, 1, 2, dtype=torch.float32, device=self.device)
        cache_out = torch.empty_like(cache)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.fe_stft_step(self._h, _ptr(wav_in), wav_in.stride(0) if B > 1 else c.hop_size, _ptr(cache),
                                             _ptr(cache_out), _ptr(spec), B, _stream(self.device)), "fe_stft_step")
        return spec, cache_out

    def istft_step(self, spec: Tensor, cache: Tensor) -> Tuple[Tensor, Tensor]:
        """ONNXSTFT.inverse: spec [B, N/2+1, 1, 2], cache [B, N-H] -> (wav_out [B, H], cache'); inputs untouched."""
        self._require_gpu()
        B, c = spec.shape[0], self.cfg
        spec = spec.to(self.device, torch.float32).contiguous()
        cache = cache.to(self.device, torch.float32).contiguous()
        assert tuple(spec.shape) == (B, c.n_fft // 2 + 1, 1, 2) and tuple(cache.shape) == (B, c.cache_len)
        wav = torch.empty(B, c.hop_size, dtype=torch.float32, device=self.device)
        cache_out = torch.empty_like(cache)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.fe_istft_step(self._h, _ptr(spec), _ptr(cache), _ptr(cache_out), _ptr(wav), c.hop_size, B,
                                              _stream(self.device)), "fe_istft_step")
        return wav, cache_out

    def stft_offline(self, x: Tensor, discard_last: bool, compress: bool = True) -> Tensor:
        """CompressedSTFT.forward: x [B, Tw] or [B, 1, Tw] -> [B, F, T, 2], T = 1 + Tw // H."""
        self._require_gpu()
        if x.dim() == 3:
            x = x.squeeze(1)
        x = x.to(self.device, torch.float32).contiguous()
        B, Tw = x.shape
        c = self.cfg
        F = c.n_fft // 2 + (0 if discard_last else 1)
        spec = torch.empty(B, F, 1 + Tw // c.hop_size, 2, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.fe_stft_offline(self._h, _ptr(x), B, Tw, F, int(compress), _ptr(spec), _stream(self.device)), "fe_stft_offline")
        return spec

    def istft_offline(self, spec: Tensor, compress: bool = True) -> Tensor:
        """CompressedSTFT.inverse: spec [B, F, T, 2] (compressed domain) -> wav [B, H * (T - 1)]."""
        self._require_gpu()
        spec = spec.to(self.device, torch.float32).contiguous()
        B, F, T, two = spec.shape
        c = self.cfg
        assert two == 2
        wav = torch.empty(B, c.hop_size * (T - 1), dtype=torch.float32, device=self.device)
        frames = torch.empty(B * T * c.n_fft, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.fe_istft_offline(self._h, _ptr(spec), B, T, F, int(compress), _ptr(wav), _ptr(frames),
                                                 _stream(self.device)), "fe_istft_offline")
        return wav

    def poison_lds(self) -> None:
        """fe_debug_poison_lds: NaN into every CU's LDS (test support: what an earlier kernel leaves in LDS must not matter)."""
        self._require_gpu()
        with torch.cuda.device(self.device):
            _lib.check(self.lib.fe_debug_poison_lds(_stream(self.device)), "fe_debug_poison_lds")

    def profile_step(self, wav_in: Tensor, state: Tensor, T: int = 1) -> Tensor:
        """Phase cycle counters (int64[64]) of workgroup 0 for the last frame of the launch."""
        self._require_gpu()
        B = wav_in.shape[0]
        H = self.cfg.hop_size
        clk = torch.zeros(64, dtype=torch.int64, device=wav_in.device)
        out = torch.empty(B, T * H, dtype=torch.float32, device=wav_in.device)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.fe_profile_step(self._h, _ptr(wav_in), wav_in.stride(0), _ptr(state), _ptr(out), T * H, B, T,
                                                _ptr(clk), _stream(self.device)), "fe_profile_step")
        return clk

    def debug_stages(self) -> List[Tuple[str, int, int, int]]:
        out = []
        for i in range(self.lib.fe_debug_stages(self._h)):
            name, r, c, off = c_char_p(), c_int(), c_int(), c_size_t()
            _lib.check(self.lib.fe_debug_stage(self._h, i, byref(name), byref(r), byref(c), byref(off)), "fe_debug_stage")
            out.append((name.value.decode(), r.value, c.value, int(off.value)))
        return out

    def debug_step(self, wav_in: Tensor, state: Tensor) -> Tuple[Tensor, Dict[str, Tensor]]:
        self._require_gpu()
        B = wav_in.shape[0]
        H = self.cfg.hop_size
        n = int(self.lib.fe_debug_floats(self._h))
        dbg = torch.zeros(B, n, dtype=torch.float32, device=wav_in.device)
        wav_out = torch.empty(B, H, dtype=torch.float32, device=wav_in.device)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.fe_debug_step(self._h, _ptr(wav_in), wav_in.stride(0), _ptr(state), _ptr(wav_out), H, B,
                                              _ptr(dbg), _stream(self.device)), "fe_debug_step")
        taps = {}
        for name, r, c, off in self.debug_stages():
            taps[name] = dbg[:, off:off + r * c].view(B, r, c)
        return wav_out, taps
