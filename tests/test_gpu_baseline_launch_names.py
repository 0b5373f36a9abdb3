"""What fe_last_step_kernel reports for every streaming entry point of BSRNN, FSPEN and LiSenNet below one stream per CU.

One launcher per family (Impl::launch_step) serves fe_step, fe_step_pool and fe_step_pool_streams[_pinned]; which kernels it picks and what it
calls them is pinned here as literals.  They were written down from the name tables and ternaries of the three launchers per family that the
one launcher replaced, not from a run.  2 streams and T <= 2 reach every branch these entry points can take at that size; the names above it
("two workgroups per CU", persistent grids) are pinned by the static_asserts of the kernel headers and by
test_c_abi_errors.py::test_last_step_kernel_names_what_was_dispatched.  Outputs are compared bit for bit elsewhere (test_gpu_step_pool.py,
test_gpu_pool_streams.py, test_gpu_step_backlog.py, test_gpu_parity.py).

Every model gets a fresh engine (seeded random weights): BSRNN's plan depends on whether the handle's three-launch scratch has been sized."""
import pytest
import torch

from common import hip_model
from test_gpu_step_chunk import _dev
from test_gpu_stream_packets import _audio, _desc

pytestmark = pytest.mark.gpu

N, CAP, SLOTS = 2, 5, [3, 1]

MLP = "bsrnn_mlp_kernel<one 16-stream tile per workgroup>"


def _engine(name):
    return hip_model(name, device=_dev()).engine


def _names(eng, shape, T):
    """the three entry points' answers for 2 streams of T hops: fe_step, fe_step_pool, fe_step_pool_streams (float32, device),
    fe_step_pool_streams_pinned (int16) - each without the ' [shape ...]' tail, which is checked here"""
    H = eng.cfg.hop_size
    got = []

    def note():
        k = eng.last_step_kernel()
        tail = f" [shape {shape}]"
        assert k.endswith(tail), k
        got.append(k[:-len(tail)])

    eng.step(torch.zeros(N, T * H, device=_dev()), eng.new_state(N), T=T)
    note()
    eng.step_pool(torch.zeros(N, T * H, device=_dev()), eng.new_state(CAP), CAP, SLOTS, T=T)
    note()
    d = _desc([(SLOTS[i], T, i * T * H, i * T * H) for i in range(N)])
    eng.step_pool_streams(_audio((N * T * H,), torch.float32, False, fill=0.0), eng.new_state(CAP), CAP, d, _audio((N * T * H,), torch.float32, False, fill=0.0), T_max=T)
    note()
    eng.step_pool_streams_pinned(_audio((N * T * H,), torch.int16, True, fill=0), eng.new_state(CAP), CAP, d, _audio((N * T * H,), torch.int16, True, fill=0), T_max=T)
    note()
    torch.cuda.synchronize()
    return got


@pytest.mark.parametrize("name,kernel", [("fspen", "fspen_frame_kernel"), ("lisennet", "lisennet_frame_kernel")])
def test_fspen_and_lisennet_run_one_kernel_named_after_the_entry_point(name, kernel):
    eng = _engine(name)
    for T in (1, 2):
        assert _names(eng, name, T) == [kernel, kernel + "<slots>", kernel + "<slots, streams>", kernel + "<slots, streams, pinned, s16>"], T


def test_bsrnn_names_follow_the_scratch_the_hop_count_and_the_role_split():
    eng = _engine("bsrnn_xxt")
    H = eng.cfg.hop_size

    def pooled(T):
        """fe_step_pool and the two packet steps only: fe_step would size the scratch"""
        got = []
        eng.step_pool(torch.zeros(N, T * H, device=_dev()), eng.new_state(CAP), CAP, SLOTS, T=T)
        got.append(eng.last_step_kernel())
        d = _desc([(SLOTS[i], T, i * T * H, i * T * H) for i in range(N)])
        eng.step_pool_streams(_audio((N * T * H,), torch.float32, False, fill=0.0), eng.new_state(CAP), CAP, d, _audio((N * T * H,), torch.float32, False, fill=0.0), T_max=T)
        got.append(eng.last_step_kernel())
        eng.step_pool_streams_pinned(_audio((N * T * H,), torch.int16, True, fill=0), eng.new_state(CAP), CAP, d, _audio((N * T * H,), torch.int16, True, fill=0), T_max=T)
        got.append(eng.last_step_kernel())
        torch.cuda.synchronize()
        return got

    # a pool state the three-launch scratch was never sized for: one kernel walks the frame
    assert pooled(1) == ["bsrnn_frame_kernel<per-hop, slots> [shape xxt]", "bsrnn_frame_kernel<per-hop, slots, streams> [shape xxt]",
                         "bsrnn_frame_kernel<per-hop, slots, streams, pinned, s16> [shape xxt]"]
    assert pooled(2) == ["bsrnn_frame_kernel<generic, slots> [shape xxt]", "bsrnn_frame_kernel<generic, slots, streams> [shape xxt]",
                         "bsrnn_frame_kernel<generic, slots, streams, pinned, s16> [shape xxt]"]
    # fe_state_init sizes it: the per-hop step in three launches, the role-split kernel first
    eng.init_state(eng.new_state(CAP), CAP)
    assert _names(eng, "xxt", 1) == [
        f"bsrnn_ov_kernel + {MLP} + bsrnn_frame_kernel<PART 2>",
        f"bsrnn_ov_kernel<slots> + {MLP} + bsrnn_frame_kernel<PART 2, slots>",
        f"bsrnn_ov_kernel<slots, streams> + {MLP} + bsrnn_frame_kernel<PART 2, slots, streams>",
        f"bsrnn_ov_kernel<slots, streams, pinned, s16> + {MLP} + bsrnn_frame_kernel<PART 2, slots, streams, pinned, s16>"]
    assert _names(eng, "xxt", 2) == ["bsrnn_frame_kernel<generic>", "bsrnn_frame_kernel<generic, slots>", "bsrnn_frame_kernel<generic, slots, streams>",
                                     "bsrnn_frame_kernel<generic, slots, streams, pinned, s16>"]
    # without the role-split kernel: the phase-by-phase PART 1
    eng.set_option("bsrnn_role_split", 0)
    assert _names(eng, "xxt", 1) == [
        f"bsrnn_frame_kernel<PART 1> + {MLP} + bsrnn_frame_kernel<PART 2>",
        f"bsrnn_frame_kernel<PART 1, slots> + {MLP} + bsrnn_frame_kernel<PART 2, slots>",
        f"bsrnn_frame_kernel<PART 1, slots, streams> + {MLP} + bsrnn_frame_kernel<PART 2, slots, streams>",
        f"bsrnn_frame_kernel<PART 1, slots, streams, pinned, s16> + {MLP} + bsrnn_frame_kernel<PART 2, slots, streams, pinned, s16>"]
