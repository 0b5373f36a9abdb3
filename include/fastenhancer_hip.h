/*
 * fastenhancer_hip.h — C ABI of libfastenhancer_hip.so (MI355X / gfx950).
 *
 * The reference (aask1357/fastenhancer) has no FFI: its inference boundary is the
 * Python call surface of
 *   - scripts/export_onnx.py:38-58      class Model: forward(wav_in, cache_stft, cache_istft, *cache_model)
 *   - models/fastenhancer/default/model.py:677-710   ONNXModel.forward(spec, *cache)   (spec -> spec)
 *   - models/fastenhancer/default/model.py:614-618   ONNXModel.initialize_cache
 *   - functional/audio_modules.py:238-303            ONNXSTFT.initialize_cache / forward / inverse
 *   - models/fastenhancer/default/model.py:532-608   remove_weight_reparameterizations (done on the host,
 *                                                    fastenhancer_amd/weights.py; this library takes FUSED weights)
 * This header is what a binding for that surface calls.  Plain C types only:
 * device pointers are raw `float*`, the stream is a `hipStream_t` passed as `void*`.
 *
 * Ownership: the caller allocates and frees every device buffer.  The handle owns only its packed
 * copy of the weights and constant tables.  All compute entry points are asynchronous on the given
 * stream and return FE_OK or a negative code; fe_last_error() gives the text (thread-local).
 * A handle is bound to the device that was current at fe_create(); it is not thread-safe, and its launches must be
 * stream-ordered: the handle owns per-workgroup scratch and frame counters, so two compute calls on the same handle may
 * not run concurrently on different HIP streams (use one handle per stream).
 */
#ifndef FASTENHANCER_HIP_H
#define FASTENHANCER_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FE_OK 0
#define FE_ERR_INVALID_ARG (-1)
#define FE_ERR_UNSUPPORTED_CONFIG (-2)
#define FE_ERR_HIP (-3)
#define FE_ERR_NO_WEIGHTS (-4)

#define FE_ARCH_FASTENHANCER 0 /* models/fastenhancer/default/model.py */
#define FE_ARCH_BSRNN 1        /* models/bsrnn/model.py: channels = num_channels, rf_blocks = num_layers */
#define FE_ARCH_FSPEN 2        /* models/fspen/model.py (configs/others/fspen.yaml): channels = channels[-1], kernel_size / n_kernels / stride
                                * as in the yaml, rf_channels / rf_freq / rf_blocks / rf_heads = dpe_kwargs channels / freq / num_blocks / groups */

#define FE_ARCH_LISENNET 3     /* models/lisennet/model.py (configs/others/lisennet.yaml): channels = num_channels, rf_blocks = n_blocks */

#define FE_MAX_KERNELS 8

/* Mirror of the yaml `model_kwargs` that select the architecture
 * (configs/fastenhancer/b.yaml:2-29; defaults models/fastenhancer/default/model.py:384-419).
 * Invariants of every shipped yaml are asserted by fe_create(): stride 4, kernel_size[0] 8 and 3
 * afterwards, window hann, stft_normalized False, resnet False, weight reparameterisations already
 * removed (fused weights).  activation and mask (every shipped yaml: SiLU, null) select a kernel built
 * for them: the shipped shapes are built for SiLU / no mask; others are built on demand
 * (python -m fastenhancer_amd.build --add-shape ...,act=<name>,mask=<name>), for the default,
 * time_kernel and ln models.  A struct that is zero in the last four fields is the shipped setting.
 *
 *   activation (FE_ACT_*)    activation_param            the reference's Act(**activation_kwargs)
 *   FE_ACT_SILU        0     -                           nn.SiLU
 *   FE_ACT_RELU        1     -                           nn.ReLU
 *   FE_ACT_LEAKY_RELU  2     negative_slope (0.01)       nn.LeakyReLU(negative_slope)
 *   FE_ACT_ELU         3     alpha (1.0)                 nn.ELU(alpha)
 *   FE_ACT_GELU        4     -                           nn.GELU(approximate='none')
 *   FE_ACT_GELU_TANH   5     -                           nn.GELU(approximate='tanh')
 *   mask (FE_MASK_*): FE_MASK_NONE 0 (mask: null), FE_MASK_SIGMOID 1, FE_MASK_TANH 2 - applied to the two
 *   dec_post channels before the complex multiply (model.py:397-404, 671).  activation_param is taken as given
 *   (the reference's defaults are in parentheses: a caller that zeroes the struct must set them itself). */
#define FE_ACT_SILU 0
#define FE_ACT_RELU 1
#define FE_ACT_LEAKY_RELU 2
#define FE_ACT_ELU 3
#define FE_ACT_GELU 4
#define FE_ACT_GELU_TANH 5
#define FE_MASK_NONE 0
#define FE_MASK_SIGMOID 1
#define FE_MASK_TANH 2
typedef struct fe_config {
    int arch;                        /* FE_ARCH_* */
    int n_fft, hop_size, win_size;   /* N, H, win (win <= N, N even) */
    int channels;                    /* C1 */
    int n_kernels;                   /* len(kernel_size) */
    int kernel_size[FE_MAX_KERNELS]; /* [8,3,3] ... */
    int stride;                      /* 4 */
    int rf_channels, rf_freq, rf_blocks, rf_heads; /* C2, F2, K, NH */
    float input_compression;         /* 0.3 */
    int kernel_size_time;            /* `model: fastenhancer.time_kernel` (models/fastenhancer/time_kernel/model.py): time taps of
                                      * the causal k = 3 Conv2d layers (3 in configs/ablation/time_kernel_b.yaml); 0 or 1 = the
                                      * default model.  The state then also holds the convs' (kernel_size_time - 1)-frame input
                                      * caches: ... | K x h | 2 (n_kernels - 1) x [B, kernel_size_time - 1, F1, C1] (encoder layers, then
                                      * decoder layers; fe_spec_step's h_dev likewise: K x h, then the caches) */
    int channels_frnn;               /* `model: fastenhancer.dprnn` (models/fastenhancer/dprnn/model.py:135-247; configs/ablation/dprnn_*.yaml):
                                      * hidden units per direction of the bidirectional sub-band GRU that replaces the attention
                                      * (must be rf_channels / 2, as in every shipped yaml); 0 = the default RNNFormer block.
                                      * rf_heads is ignored.  Weight sections: rf_block.k.frnn.{weight,bias}_{ih,hh}_l0[_reverse],
                                      * rf_block.k.frnn_fc.{weight,bias} instead of attn.qkv / attn_fc, no pe; state as the default model */
    int lookbehind;                  /* `model: fastenhancer.dptransformer` (models/fastenhancer/dptransformer/model.py; configs/ablation/dpt_*.yaml):
                                      * frames of history of the causal time attention that replaces the time GRU (31 in every shipped
                                      * yaml, the only value compiled); 0 = the default block.  Weight sections: time_pe [NH, L+1] (the model's
                                      * `pe`), rf_block.k.time_attn.qkv.weight instead of rnn.*.  State (and fe_spec_step's h_dev): per
                                      * block the K cache then the V cache, each [B*F2, NH, L, C2/NH] (DPTBlock.initialize_cache, :194-198),
                                      * then B floats `head`: every cache is a ring over its L slots - the frame that is t steps old sits
                                      * in slot (head + L - t) mod L, a step overwrites slot `head` and advances it (one slot written per
                                      * frame instead of the reference's shift of all L).  head = 0 (fe_state_init, or caches copied in from
                                      * the reference) is exactly the reference's tensor, oldest frame first; to read the caches back in
                                      * that order rotate each [.., L, ..] axis left by head.  A cache slot whose first K element is +inf
                                      * does not take part (how a run "without caches", :216-218, marks the frames before the start; zero
                                      * caches do take part) */
    int ln;                          /* `model: fastenhancer.ln` (models/fastenhancer/ln/model.py; configs/ablation/ln_b.yaml): 1 = GroupNorm(1, C)
                                      * after every conv and the reference's LayerNorm over (F2, C2) after the blocks' fc layers instead of
                                      * (folded) BatchNorms.  Weight sections = that model's state_dict after remove_weight_reparameterizations
                                      * (convs with their own biases, <conv>.1 / .2 / .4 and rnn_post_norm / attn_post_norm weight + bias),
                                      * the final conv as dec_post.2 with its scale folded in.  State as the default model */
    float rf_eps;                    /* ln: eps of the blocks' LayerNorms (rnnformer_kwargs.eps; 0 -> 1e-5) */
    int bidirectional;               /* `model: fastenhancer.noncausal` (models/fastenhancer/noncausal/model.py:186-187; configs/fastenhancer_dns/huge_noncausal*.yaml,
                                      * configs/fastenhancer_48khz/huge_noncausal.yaml): 1 = the blocks' time GRU is bidirectional and rnn_fc maps
                                      * 2 C2 -> C2.  Weight sections: + rf_block.k.rnn.{weight,bias}_{ih,hh}_l0_reverse, rnn_fc.weight [C2, 2 C2].
                                      * The reference module has the offline `Model` only (:348, :628-635): fe_offline is the one compute entry
                                      * point (no caches: fe_state_floats = the two STFT caches, fe_step / fe_spec_step return FE_ERR_UNSUPPORTED_CONFIG) */
    int activation;                  /* FE_ACT_* (0 = SiLU, every shipped yaml) */
    float activation_param;          /* FE_ACT_LEAKY_RELU: negative_slope, FE_ACT_ELU: alpha; ignored otherwise */
    int mask;                        /* FE_MASK_* (0 = none, every shipped yaml) */
    int resnet;                      /* must be 0: the resnet option (model.py:636-668) is not built into this library */
} fe_config;

typedef struct fe_handle fe_handle;

/* Model construction: ONNXModel.__init__ (model.py:383-521) + ONNXSTFT.__init__ window tables
 * (functional/audio_modules.py:182-236).  FE_ERR_UNSUPPORTED_CONFIG if no kernel was compiled
 * for this shape (shapes of all shipped fastenhancer yamls are compiled in). */
int fe_create(const fe_config* cfg, fe_handle** out);
void fe_destroy(fe_handle* h);

/* Fused-weight blob (what an RCCL broadcast carries).  Sections are the fused state_dict tensors
 * (SURVEY.md Appendix A.1 "Fused"), fp32, reference memory layout, concatenated in the order
 * reported by fe_weight_section(); each section offset is a multiple of 4 floats. */
size_t fe_weight_floats(const fe_handle* h);
int fe_weight_sections(const fe_handle* h);
int fe_weight_section(const fe_handle* h, int idx, const char** name, size_t* offset_floats, size_t* count_floats);
/* load_state_dict (wrappers/ns.py:308-314) for already-fused weights: blob_dev is a DEVICE pointer.
 * Synchronises the stream (load-time only); repacks into MFMA fragment order inside the handle. */
int fe_load_weights(fe_handle* h, const float* blob_dev, size_t nfloats, void* stream);

/* Per-stream state = the reference's cache list, concatenated:
 *   cache_stft  [B, N-H] | cache_istft [B, N-H] | K x h [1, B*F2, C2]
 * (scripts/export_onnx.py:43-46).  fe_state_init zeroes it (initialize_cache).  The model part (what fe_spec_step takes as
 * h_dev) per architecture, every tensor sized for B streams and laid out as the reference's:
 *   FE_ARCH_FASTENHANCER  K x h [1, B*F2, C2]  (kernel_size_time > 1: + the conv caches, see fe_config)
 *   FE_ARCH_BSRNN         2 * num_layers x [B*31, 2C]: h0, c0, h1, c1, ...              (models/bsrnn/model.py:409-416)
 *   FE_ARCH_FSPEN         num_blocks * groups x [1, B*freq/groups, C] inter-GRU states  (models/fspen/model.py:293-297)
 *   FE_ARCH_LISENNET      [B,1,257] phase | [B,4,1,257] [B,8,1,128] [B,12,1,64] encoder frames | n_blocks x ([1,B*32,24] GRU,
 *                         [B,32,2,32] ConvGLU frames) | [B,4,1,256] decoder frame     (models/lisennet/model.py:380-396)
 * FE_ARCH_BSRNN: fe_state_init also sizes the handle's scratch for the per-hop step of B streams (that step runs as three launches with
 * 10.6 KB per stream between them); a step of a larger batch than any fe_state_init has seen grows it on its first call (a device
 * allocation: not inside a stream capture).  FE_ARCH_FSPEN / FE_ARCH_LISENNET likewise from their "..._stream_batch_min" streams (LiSenNet, r6: three
 * launches with 49 KB per stream between them - the activation tensors of each sixteen-stream tile in the layout the matrix-core kernel reads). */
size_t fe_state_floats(const fe_handle* h, int B);
int fe_state_init(fe_handle* h, float* state_dev, int B, void* stream);

/* The wav->wav streaming step, scripts/export_onnx.py:48-58, for B independent streams and T
 * consecutive hops per stream (T=1: one hop, as scripts/test_onnx.py:44-50 drives it).
 *   wav_in [b*in_stride + t*H + n], wav_out [b*out_stride + t*H + n],  n < H, t < T, b < B.
 * The state is updated in place. */
int fe_step(fe_handle* h, const float* wav_in_dev, size_t in_stride, float* state_dev,
            float* wav_out_dev, size_t out_stride, int B, int T, void* stream);

/* The same step for n of the streams of a state buffer sized for `capacity` streams (fe_state_floats(h, capacity), every tensor of
 * the layout above sized for `capacity`): stream i of the call (i < n) is state slot slots_dev[i]; wav_in / wav_out rows are in call
 * order, as for fe_step (row i = wav_in [i*in_stride + t*H + k]).  The state of slots not named is left untouched, so streams can join
 * and leave a batch without copying state.
 *   slots_dev: a DEVICE int32 array of n entries, read by the kernel when it runs (a captured graph may serve other streams on each
 *     replay after its contents are rewritten).  Its contents are not checked on the host.  Duplicate slots are undefined.  A slot
 *     outside [0, capacity) touches no state: its stream's wav_out rows are zero.
 *   The host checks 1 <= n <= capacity, T >= 1, non-null pointers and the strides as fe_step does.  The kernel is the one fe_step(B = n)
 *     picks (fe_last_step_kernel names its slotted form, "... slots>"); the results of each stream are those of fe_step on a state
 *     holding only the named slots, bit for bit.
 *   FastEnhancer family only (the default, time_kernel, ln, dprnn and dptransformer models): BSRNN, FSPEN and LiSenNet return
 *     FE_ERR_UNSUPPORTED_CONFIG, and so does the noncausal model, as for fe_step. */
int fe_step_slots(fe_handle* h, const float* wav_in_dev, size_t in_stride, float* state_dev, int capacity, const int* slots_dev,
                  float* wav_out_dev, size_t out_stride, int n, int T, void* stream);
/* fe_step_slots for EVERY family with a streaming state: what a pool of live streams calls.  Signature, row layout, slot rules (slots_dev is
 * device int32 read when the kernels run, unchecked on the host; a slot outside [0, capacity) touches no state and its T output rows are zero;
 * duplicates are undefined; slots not named keep their bits) and host checks (same codes, same wording, before any device work) are
 * fe_step_slots'.
 *   FastEnhancer models: the call IS fe_step_slots - same launch, same bits, same refusals, same fe_last_step_kernel.  The noncausal model:
 *     FE_ERR_UNSUPPORTED_CONFIG with fe_step's message.
 *   FE_ARCH_BSRNN / FE_ARCH_FSPEN / FE_ARCH_LISENNET: the PER-STREAM kernels fe_step(B = n, T) picks, in slotted instantiations that take every
 *     state address from (slots_dev[i], capacity) - BSRNN's role-split or phase-by-phase PART 1 (fe_set_step_kernel, "bsrnn_role_split"), its
 *     three-launch step (each launch reads slots_dev itself), the single-kernel walk for T > 1, the persistent forms above the streams resident
 *     at once.  The stream-batched forms (bsrnn_sb_*, "bsrnn_fused_step", FSPEN's and LiSenNet's *_sb_* middle) are never taken, at any n and
 *     whatever the "..._stream_batch_min" options say: their tensors are laid out per call tile.  fe_last_step_kernel: "... slots>".
 *     Each named stream's wav_out rows and state are those of fe_step(B = n, T) under the same per-stream kernel on a dense state holding the
 *     named slots' records, bit for bit.
 *   The call allocates nothing, is asynchronous on `stream` and can be captured in a graph.  BSRNN's three-launch step passes 10.6 KB per stream
 *     through the scratch that fe_state_init(h, state, capacity) sized (see above), as fe_step does; where no fe_state_init of the handle has
 *     sized it for n streams, the step runs the single-kernel walk instead of growing it. */
int fe_step_pool(fe_handle* h, const float* wav_in_dev, size_t in_stride, float* state_dev, int capacity, const int* slots_dev,
                 float* wav_out_dev, size_t out_stride, int n, int T, void* stream);
/* What fe_state_init writes (zeros), for the named slots only: a stream joining.  slots_dev, capacity, duplicates and the families as for
 * fe_step_slots; out-of-range slots are skipped. */
int fe_state_reset_slots(fe_handle* h, float* state_dev, int capacity, const int* slots_dev, int n, void* stream);

/* Moving live streams between state buffers.  The STATE RECORD of a stream is fe_state_floats(h, 1) floats: exactly the state buffer of a
 * capacity-1 batch holding that stream, in the layout above - the reference's cache list for one stream.  It is no new format: a record can be
 * handed to fe_step(B = 1) as it stands; n records lie back to back, records[i * fe_state_floats(h, 1) + ...]; every state is a list of tensors
 * [rows][capacity][len], so fe_state_floats(h, B) = B * fe_state_floats(h, 1) for every family.  dptransformer rings are copied verbatim
 * together with the stream's `head` (no rotation; a +inf "slot not in use" mark survives).  A record is valid for handles of the same
 * fe_config and library version, on any device; it is not portable across shapes.
 *   export: records[i] = the state of slot slots_dev[i] of state_dev (sized for `capacity`); state_dev is not written.  A slot outside
 *     [0, capacity) yields the record fe_state_init leaves (zeros).
 *   import: slot slots_dev[i] of state_dev = records[i], with no reset first; no other float of state_dev is written.  A slot outside
 *     [0, capacity) is skipped: nothing is written anywhere.  Duplicate slots are undefined.
 *   Families: every family with a streaming state - the FastEnhancer default, time_kernel, ln, dprnn and dptransformer models, BSRNN, FSPEN
 *     and LiSenNet; for the last three, slot s is stream s of a state that plain fe_step(B = capacity) steps (the slotted STEPS stay
 *     FastEnhancer's).  The noncausal model returns FE_ERR_UNSUPPORTED_CONFIG, as for fe_step.  Scratch the handle owns (BSRNN's inter-launch
 *     buffers, the rings of fe_spec_step) is not state and is not touched.  Weights need not be loaded.
 *   slots_dev: a DEVICE int32 array of n entries, read by the kernel when it runs (a captured graph may move other streams on each replay);
 *     its contents are not checked on the host.
 *   records: device memory of the current device, or page-locked HOST memory mapped for it (the pinning rule of fe_step_slots_pinned), which
 *     the kernel reads or writes directly over PCIe.  The first and last float of the range are looked up before anything is launched:
 *     pageable memory is FE_ERR_INVALID_ARG.  Any 4-byte alignment is legal (16-byte loads and stores are used where both sides allow).
 *     records overlapping state_dev is undefined.
 *   The host checks non-null pointers and 1 <= n <= capacity before any device work.  One launch, asynchronous on `stream`; for host records
 *     the completion rule of fe_step_slots_pinned applies.  fe_last_step_kernel is not affected. */
int fe_state_export_slots(fe_handle* h, const float* state_dev, int capacity, const int* slots_dev, float* records, int n, void* stream);
int fe_state_import_slots(fe_handle* h, float* state_dev, int capacity, const int* slots_dev, const float* records, int n, void* stream);

/* fe_step / fe_step_slots for audio in PAGE-LOCKED HOST memory: one launch whose kernel reads each hop over PCIe and writes the enhanced
 * hop back there - no staging buffers, copies or events, and one node when captured into a graph.  Row layout, strides, families, slot
 * rules and the kernel choice are those of fe_step_slots (fe_step_pinned: capacity = B, stream i = slot i); the results are theirs on
 * device copies of the same rows, bit for bit.  fe_last_step_kernel names the kernel with "pinned" in the brackets.
 *   Pinning rule: every float of both audio ranges must be host memory that is page-locked and mapped for the current device
 *     (hipHostMalloc / hipHostRegister; torch's pin_memory()).  The first and last float of each range are looked up before anything is
 *     launched; pageable or device memory is FE_ERR_INVALID_ARG.  state_dev and slots_dev are device memory, as for fe_step_slots.
 *   Completion rule: the call is asynchronous on `stream`.  wav_in_host must not be rewritten, nor wav_out_host read, until `stream`
 *     has completed the step (hipStreamSynchronize or an event); the output is visible to the host from then on. */
int fe_step_pinned(fe_handle* h, const float* wav_in_host, size_t in_stride, float* state_dev, float* wav_out_host, size_t out_stride,
                   int B, int T, void* stream);
int fe_step_slots_pinned(fe_handle* h, const float* wav_in_host, size_t in_stride, float* state_dev, int capacity, const int* slots_dev,
                         float* wav_out_host, size_t out_stride, int n, int T, void* stream);

/* The streaming step for PACKET audio: every stream of the call advances its own number of hops, reads and writes its audio at its own
 * place in two buffers (a service's rings), as float32 or as int16 PCM - one launch for a tick on which some streams have no complete
 * hop, most have one and some have several.  State buffer, capacity, families and the kernel choice are those of fe_step_slots(n, T = T_max).
 *   desc_dev: a DEVICE array of n descriptors, read by the kernel when it runs (a captured graph serves other streams, hop counts and
 *     offsets on each replay after its contents are rewritten); not checked on the host.
 *   Addressing: stream i reads hop t (t < hops) at wav_in [in_offset + t*H .. + H) and writes wav_out [out_offset + t*H .. + H), in ELEMENTS
 *     of `format`: FE_AUDIO_F32 floats, FE_AUDIO_S16 int16.  Any element alignment is legal; rows that are 16-byte aligned go out as
 *     16-byte stores.
 *   hops: clamped by the kernel to [0, T_max].  With 0 hops the stream neither reads nor writes audio or state.
 *   Bounds: in_count / out_count are the element counts of the two buffers.  A stream whose clamped range [offset, offset + hops*H) does
 *     not lie inside [0, count) on EITHER side is skipped like a stream with 0 hops: no audio, no state, nothing outside the buffers.  The
 *     kernel makes this check for every stream on every call.
 *   Slots: as for fe_step_slots - a slot outside [0, capacity) touches no state and its hops output rows are zero; duplicates are undefined.
 *   int16: input x = s / 32768 (exact); output q = clamp(rint(y * 32768), -32768, 32767), ties to even, NaN -> 0.  The state is float
 *     either way: the results are those of the float32 call on s / 32768, quantised on the way out.
 *   The host checks 1 <= n <= capacity, T_max >= 1, non-null pointers and the format; families as for fe_step_slots.  Each stream's rows and
 *     state are those of fe_step_slots(T = its hops) under the same kernel, bit for bit (FE_STEP_KERNEL_WAVES4 where hop counts differ: the
 *     chunked-equals-per-hop contract of fe_set_step_kernel).  fe_last_step_kernel names the kernel with "streams" (and "pinned", "s16")
 *     in the brackets.
 * fe_step_streams_pinned: wav_in / wav_out are page-locked HOST memory, read and written by the kernel over PCIe - the pinning and completion
 *   rules of fe_step_slots_pinned, checked for [wav, wav + count) of each buffer; the in-kernel bounds check is the same. */
typedef struct fe_stream_desc {      /* 24 bytes */
    int slot;                        /* state slot */
    int hops;                        /* hops this stream advances in this call */
    long long in_offset;             /* element offset of its first input sample from wav_in */
    long long out_offset;            /* element offset of its first output sample from wav_out */
} fe_stream_desc;
#define FE_AUDIO_F32 0
#define FE_AUDIO_S16 1               /* int16 PCM, full scale 32768 */
/* G.711, one unsigned byte per sample - formats of the RESAMPLER only ("Audio at another sample rate", below); every model step refuses
 * them as it refuses any format but the two above.  Codes 2 and 3 are not formats. */
#define FE_AUDIO_ULAW  4             /* G.711 mu-law (PCMU) */
#define FE_AUDIO_ALAW  5             /* G.711 A-law (PCMA) */
int fe_step_streams(fe_handle* h, const void* wav_in_dev, size_t in_count, float* state_dev, int capacity, const fe_stream_desc* desc_dev,
                    void* wav_out_dev, size_t out_count, int n, int T_max, int format, void* stream);
int fe_step_streams_pinned(fe_handle* h, const void* wav_in_host, size_t in_count, float* state_dev, int capacity, const fe_stream_desc* desc_dev,
                           void* wav_out_host, size_t out_count, int n, int T_max, int format, void* stream);
/* fe_step_streams[_pinned] for EVERY family with a streaming state: what a service's packet pool calls.  It stands to fe_step_streams[_pinned] as
 * fe_step_pool stands to fe_step_slots: the same parameter lists, descriptor rules (desc_dev read by the kernels when they run, unchecked on the
 * host; hops clamped to [0, T_max]; a stream with 0 hops reads and writes nothing, no audio and no state; a stream whose clamped range
 * [offset, offset + hops*H) leaves [0, count) on either side is skipped like one with 0 hops - checked for every stream on every call; a slot
 * outside [0, capacity) touches no state and its hops output rows are zero; duplicate slots are undefined; slots the call does not advance keep
 * every bit), formats (FE_AUDIO_F32 / FE_AUDIO_S16 with the conversion rules above, any element alignment, 16-byte stores for rows that are
 * 16-byte aligned), pinning and completion rules, and host checks (same codes, same wording under this function's name, before any device work).
 *   FastEnhancer models: the call IS fe_step_streams[_pinned] - same launch, same bits, same refusals, same fe_last_step_kernel.  The noncausal
 *     model: FE_ERR_UNSUPPORTED_CONFIG with fe_step's message.  (fe_step_streams* itself keeps refusing the other families.)
 *   FE_ARCH_BSRNN / FE_ARCH_FSPEN / FE_ARCH_LISENNET: the launches fe_step_pool(n, T = T_max) picks - per-stream kernels only, never a
 *     stream-batched form - in packet instantiations that take slot, hop count and audio offsets from the stream's descriptor.  BSRNN with
 *     T_max == 1 and the scratch fe_state_init sized: the three-launch step (bsrnn_ov_kernel or PART 1, bsrnn_mlp_kernel, PART 2), each
 *     per-stream launch reading the descriptor itself and skipping a stream without a hop or with ranges outside the buffers as it skips a
 *     slot out of range (nothing is handed to the scratch; the batched MLP works on that stream's stale row, which reaches no other stream);
 *     the first launch reads the audio, the last writes it.  BSRNN otherwise: the single-kernel walk.  fe_last_step_kernel: "streams" (and
 *     "pinned", "s16") after "slots" in the brackets.
 *   wav_in and wav_out must not overlap: a later launch of the step, or another stream's workgroup, may write output while input is still read.
 *   Each stream's output rows and state are those of fe_step_pool(T = its hops) on the same slot, bit for bit wherever that call dispatches
 *     the same kernel functions: always for FSPEN and LiSenNet (one kernel for every T); for BSRNN every stream of a T_max == 1 call and every
 *     stream with 2 or more hops of a T_max > 1 call.  A BSRNN stream with 1 hop in a T_max > 1 call runs the generic walk where
 *     fe_step_pool(T = 1) runs the per-hop kernels: equal to the relative tolerance those two kernels agree to (a few float32 ulps of the
 *     waveform's scale), not bit for bit.
 *   The call allocates nothing, is asynchronous on `stream` and can be captured in a graph (BSRNN's three launches: a linear chain). */
int fe_step_pool_streams(fe_handle* h, const void* wav_in_dev, size_t in_count, float* state_dev, int capacity, const fe_stream_desc* desc_dev,
                         void* wav_out_dev, size_t out_count, int n, int T_max, int format, void* stream);
int fe_step_pool_streams_pinned(fe_handle* h, const void* wav_in_host, size_t in_count, float* state_dev, int capacity, const fe_stream_desc* desc_dev,
                                void* wav_out_host, size_t out_count, int n, int T_max, int format, void* stream);

/* The packet step with two per-stream controls, both inside the frame kernels of fe_step_streams (the same kernels, the same names from
 * fe_last_step_kernel, the same host checks, families and refusals): a limit on how far a stream may be attenuated, and input / output level meters.
 *   min_gain: [capacity] floats indexed by state SLOT, or NULL.  min_gain[slot] is a linear amplitude in [0, 1] (-20 dB = 0.1), clamped to that range
 *     by the kernel; 0 and NaN mean no limit.  With c = input_compression and M the complex mask of a bin (after the shape's mask function), the
 *     net amplitude gain of the bin is |M|^(1/c); the kernel applies M' = M max(1, m_min / |M|), m_min = min_gain^c, and M' = (m_min, 0) where
 *     |M| = 0: the phase is kept, the magnitude lifted to m_min, so no bin is attenuated by more than min_gain.  Everything downstream (complex
 *     multiply, un-compress, iSTFT; the Nyquist bin stays zero) is unchanged.  The limit touches the output path only: a stream's GRU states,
 *     K / V rings, conv caches and cache_stft are bit for bit those of the unlimited run; wav_out and cache_istft differ.  A stream with
 *     min_gain 0 (or a NULL table) takes the code path of fe_step_streams: its results are those, bit for bit.
 *   levels: [capacity] rows indexed by state SLOT, 16-byte aligned (else FE_ERR_INVALID_ARG), or NULL.  For every stream that advanced at least
 *     one hop in the call the kernel writes row `slot`, as one 16-byte store: the sum of squares and the largest |x| of its hops * H input
 *     samples as floats (int16: s / 32768), and of its hops * H output samples as floats, before the int16 quantisation.  Not written: the
 *     rows of streams with 0 hops, of streams skipped by the bounds check, of slots outside [0, capacity), and of slots the call does not
 *     name.  No atomics and a fixed order of combination: a row is bitwise reproducible from run to run and does not depend on the stream's
 *     position in the batch, on device or pinned audio, or on int16 against float32 on s / 32768.  Peaks are exact; sums are fp32 sums.
 *   Memory: both tables are device memory, or page-locked host memory mapped for the device; pass either kind as it is (a host pointer or
 *     its device view).  Every call looks both ends of each non-NULL table up (hipPointerGetAttributes, and hipHostGetDevicePointer for host
 *     memory: host time on the calling thread, no device time), hands the kernel the device view, and refuses memory the device cannot
 *     reach, or a table that spans two allocations, with FE_ERR_INVALID_ARG before any launch.  The kernel reads min_gain when it runs: a
 *     captured graph follows a rewritten table.  Level rows in host memory are visible once `stream` has completed.
 * With both tables NULL the calls are fe_step_streams / fe_step_streams_pinned. */
typedef struct fe_stream_levels { float in_sumsq, in_peak, out_sumsq, out_peak; } fe_stream_levels;   /* 16 bytes */
int fe_step_streams_ctl(fe_handle* h, const void* wav_in_dev, size_t in_count, float* state_dev, int capacity, const fe_stream_desc* desc_dev,
                        void* wav_out_dev, size_t out_count, int n, int T_max, int format, const float* min_gain, fe_stream_levels* levels,
                        void* stream);
int fe_step_streams_ctl_pinned(fe_handle* h, const void* wav_in_host, size_t in_count, float* state_dev, int capacity,
                               const fe_stream_desc* desc_dev, void* wav_out_host, size_t out_count, int n, int T_max, int format,
                               const float* min_gain, fe_stream_levels* levels, void* stream);
/* The two controls for EVERY family with a streaming state: fe_step_pool_streams[_pinned] with the two tables of fe_step_streams_ctl.  The
 * parameter lists are those of fe_step_streams_ctl[_pinned].  Descriptor rules, in-kernel bounds check, formats, pinning and completion rules, kernel
 * choice, fe_last_step_kernel's strings and "allocates nothing, capturable" are those of fe_step_pool_streams[_pinned]; the tables are those of
 * fe_step_streams_ctl - slot-indexed, [capacity], device or mapped page-locked host memory, both ends looked up on every call, levels 16-byte
 * aligned, read and written when the kernels run - with the same codes and wording under these names.
 *   FastEnhancer models: the call IS fe_step_streams_ctl[_pinned] - same launch, bits, refusals and fe_last_step_kernel; the noncausal model gets
 *     fe_step's refusal.  (fe_step_streams_ctl* itself keeps refusing the other families.)
 *   Both tables NULL: the call is fe_step_pool_streams[_pinned] - the same code path, the same bits.
 *   min_gain on BSRNN, FSPEN and LiSenNet: their outputs are not a mask times the input (BSRNN's is X M + R with an additive residual, FSPEN
 *     combines two masks), so a floor on a mask bounds nothing.  The limit is on the output bin against the input bin.  g = min_gain[slot],
 *     clamped to [0, 1] by the kernel (NaN and 0: off); c = input_compression, m = g^c.  Per frame, for all 257 bins, with X_c the compressed
 *     input bin the model saw and Y_c the bin it produced in the compressed domain, right before the un-compress:
 *       Y_c' = Y_c max(1, m |X_c| / |Y_c|),   and   Y_c' = m X_c (the input's phase) where |Y_c|^2 < FLT_MIN.
 *     Un-compress and iSTFT follow unchanged; after the un-compress |Y| >= g max(|X|, 1e-5): no bin leaves attenuated by more than min_gain.
 *     For a pure complex mask this is FastEnhancer's floor in value, not in bits (FastEnhancer keeps its own).  The limit touches the output
 *     path only: every state tensor but cache_istft holds the bits of the unlimited run.  A stream whose gain is off takes the code path of
 *     fe_step_pool_streams: its rows and state are those, bit for bit.
 *   levels: as for fe_step_streams_ctl - for every stream that advanced at least one hop, row `slot` is (sum of squares, max |x|) of its
 *     hops * H input samples as floats (int16: s / 32768) and of its hops * H output samples as floats before quantisation; peaks exact, sums
 *     fp32 sums without atomics in a fixed order; a row is bitwise reproducible and does not depend on the stream's position in the batch, on
 *     device or pinned audio, or on int16 against float32 of s / 32768.  Rows of streams with 0 hops, of streams skipped by the bounds check, of
 *     slots outside [0, capacity) and of slots not named keep every bit.  FSPEN, LiSenNet and BSRNN's single-kernel walk write the row as one
 *     16-byte store at the end of the stream.  BSRNN's three-launch step (T_max == 1) writes it as two 8-byte halves: the launch that reads
 *     the audio (bsrnn_ov_kernel or PART 1) stores the input half, PART 2 the output half - the one-store promise is NOT made for this step;
 *     the row is complete once `stream` has completed the call.
 *   Weight banks stay FastEnhancer's.  A stream that comes back with a backlog: fe_step_pool_streams_chunk, below. */
int fe_step_pool_streams_ctl(fe_handle* h, const void* wav_in_dev, size_t in_count, float* state_dev, int capacity, const fe_stream_desc* desc_dev,
                             void* wav_out_dev, size_t out_count, int n, int T_max, int format, const float* min_gain, fe_stream_levels* levels,
                             void* stream);
int fe_step_pool_streams_ctl_pinned(fe_handle* h, const void* wav_in_host, size_t in_count, float* state_dev, int capacity,
                                    const fe_stream_desc* desc_dev, void* wav_out_host, size_t out_count, int n, int T_max, int format,
                                    const float* min_gain, fe_stream_levels* levels, void* stream);

/* Weight banks: the streams of one packet batch on different checkpoints of the handle's shape (a canary, per-customer fine-tunes, a roll-out
 * under live streams) - one handle, one state buffer and one launch per tick for all of them.
 *   The banks of a handle sit in ONE device allocation, n_banks packed buffers at a fixed stride (the packed size rounded up, so that every
 *     bank base keeps the alignment of the kernels' 16-byte fetches).  Bank 0 is what fe_load_weights loads and what every other entry point
 *     reads: fe_step*, fe_step_slots*, fe_step_streams[_ctl][_pinned], fe_step_chunk, fe_spec_step and fe_offline keep their results bit for bit.
 *   fe_set_weight_banks: 1 (what fe_create leaves) .. FE_MAX_WEIGHT_BANKS, else FE_ERR_INVALID_ARG.  The contents of the banks that survive,
 *     [0, min(old, new)), are kept.  Like fe_load_weights it may synchronise `stream` and allocates: load-time work, not inside a capture.
 *     Arguments are checked before any device work.  n_banks > 1 is for the FastEnhancer streaming models (default, time_kernel, ln, dprnn,
 *     dptransformer); BSRNN, FSPEN, LiSenNet and the noncausal model get FE_ERR_UNSUPPORTED_CONFIG with a message that names the family;
 *     n_banks == 1 is FE_OK for all of them.
 *   fe_load_weights_bank: fe_load_weights into bank `bank` (outside [0, n_banks): FE_ERR_INVALID_ARG), in place: no other bank's bytes are
 *     written and the allocation does not move, so a launch that reads other banks and was enqueued earlier on the same stream stays valid -
 *     load bank k while the others serve.  fe_load_weights(h, ...) is fe_load_weights_bank(h, 0, ...).
 *   fe_step_streams_banked[_pinned]: fe_step_streams_ctl[_pinned] with one more slot-indexed table.
 *     bank: [capacity] int32 indexed by state SLOT, or NULL: bank[slot] names the bank the stream of that slot runs on.  Device memory or
 *       page-locked host memory mapped for the device, looked up and refused as min_gain is.  The kernel reads the table when it runs: a
 *       captured graph follows a rewritten table.
 *     bank == NULL: the call is fe_step_streams_ctl[_pinned] - the same code path, the same bits.
 *     FE_ERR_NO_WEIGHTS unless EVERY bank 0 .. n_banks - 1 is loaded (the host cannot see the table's contents).
 *     A stream whose bank[slot] lies outside [0, n_banks) is treated as a stream whose slot lies outside [0, capacity): its output rows are
 *       zero, no state is touched and no level row is written.
 *     Each stream's output rows, state and level row are, bit for bit, what fe_step_streams_ctl gives that stream on a one-bank handle loaded
 *       with its bank's checkpoint, under the same kernel.  fe_last_step_kernel adds "banks" inside the brackets (after "streams" / "pinned" /
 *       "s16") when bank != NULL.
 *     Moving a live stream from one bank to another is allowed (the state layout is the same) and undefined beyond "no fault". */
#define FE_MAX_WEIGHT_BANKS 64
int fe_set_weight_banks(fe_handle* h, int n_banks, void* stream);
int fe_weight_banks(const fe_handle* h);
int fe_load_weights_bank(fe_handle* h, int bank, const float* blob_dev, size_t nfloats, void* stream);
int fe_step_streams_banked(fe_handle* h, const void* wav_in_dev, size_t in_count, float* state_dev, int capacity, const fe_stream_desc* desc_dev,
                           void* wav_out_dev, size_t out_count, int n, int T_max, int format, const float* min_gain, fe_stream_levels* levels,
                           const int* bank, void* stream);
int fe_step_streams_banked_pinned(fe_handle* h, const void* wav_in_host, size_t in_count, float* state_dev, int capacity,
                                  const fe_stream_desc* desc_dev, void* wav_out_host, size_t out_count, int n, int T_max, int format,
                                  const float* min_gain, fe_stream_levels* levels, const int* bank, void* stream);

/* The same step for callers whose audio lives in HOST memory (the reference's scripts/test_onnx.py feeds numpy arrays hop by hop):
 * n_calls consecutive fe_step calls of T hops each, hop block c = hops c*T .. c*T+T-1 of
 *   wav_in_host [b*in_stride + t*H + n], wav_out_host [b*out_stride + t*H + n]   (page-locked for asynchronous copies; pageable works, slower)
 * The copy-in of block c + 1 and the copy-out of block c - 1 run under the kernel of block c: two copy streams of the handle next
 * to `stream`, double-buffered device staging in work_dev (4*B*T*H floats).  Asynchronous: `stream` is complete when the last block
 * is back in host memory.  (bench.py's `value` is the device-resident rate; this is the PCIe-inclusive one - DESIGN.md 1.) */
int fe_step_host(fe_handle* h, const float* wav_in_host, size_t in_stride, float* state_dev, float* wav_out_host,
                 size_t out_stride, int B, int T, int n_calls, float* work_dev, void* stream);

/* The spec->spec step, ONNXModel.forward (model.py:677-710): spec [B, N/2+1, T, 2] in and out,
 * h_dev = the K GRU caches [K][B*F2][C2] (updated in place).  Any T >= 1. */
int fe_spec_step(fe_handle* h, const float* spec_in_dev, float* h_dev, float* spec_out_dev,
                 int B, int T, void* stream);

/* Time pipelining of fe_offline / fe_spec_step (T >= 4 frames per stream, at most half as many streams as CUs): the
 * frames of a stream are spread over up to `frames_in_flight` co-resident workgroups that hand the GRU state of each
 * RNNFormer block from frame to frame through global memory (everything else in a frame is independent of the other
 * frames).  Negative (the default) = a width chosen from the model size (8 .. 64); 0 or 1 = off (one workgroup walks the
 * T frames of a stream); values above 64 are clamped to 64 (the per-frame rings in work_dev are sized for that).  Results agree to fp32 rounding.  BSRNN's fe_offline is pipelined the same way (the time-LSTM (h, c) of
 * each layer is the hand-off; up to 64 frames in flight), and so are the ln variant's, the time_kernel variant's and the
 * dptransformer variant's (the time convs' input frames / the K-V caches go through per-frame rings: in work_dev for fe_offline;
 * for fe_spec_step - ONNXModel.forward(spec, *caches) with T >> 1, time_kernel/model.py:746-806, dptransformer/model.py:194-236 - in a
 * grow-only buffer of the handle, filled from the caller's caches before the launch and read back after it: a first or wider call
 * allocates, so not inside a stream capture), FSPEN's (its inter-GRU states per DPE block) and LiSenNet's (its nine caches through
 * a ring of per-frame slots). */
int fe_set_time_pipeline(fe_handle* h, int frames_in_flight);

/* fe_step for FEW streams and MANY hops - a recording, or a live stream that comes back with a backlog: fe_step(h, ..., B, T, stream) with
 * the T frames of each stream spread over the time pipeline instead of walked by one workgroup.  Same rows (wav_in [b*in_stride + t*H + n],
 * wav_out likewise), same state buffer (fe_state_floats(h, B), updated in place), same argument checks, error codes and refusals as fe_step
 * (the arguments are checked before the handle's weights; the noncausal model is refused with fe_step's message).
 *   Results: those of fe_step to fp32 rounding, for wav_out and every state tensor (the frames' sums are formed in another order);
 *     cache_stft, a copy of input samples, bit for bit.  The state it leaves is valid for every other entry point: fe_step, fe_step_slots on
 *     a capacity-B buffer, export / import; a dptransformer state is a valid ring (head = 0, oldest frame first).
 *   wav_in and wav_out MUST NOT overlap (fe_step reads a hop before it writes it; here the second launch reads wav_in for the new
 *     cache_stft after the first has run).
 *   work_dev: fe_step_chunk_work_floats(h, B, T) floats of scratch - frame counters, the windowed output frames [B][T][N] and, for the
 *     time_kernel / dptransformer models, the rings their frames exchange conv inputs / K-V through.  The size depends on the model, B and
 *     T only and is monotone in both: a buffer sized for (B, T) serves every call with at most B streams and at most T hops, whatever
 *     fe_set_time_pipeline says.  It is an argument, not a buffer of the handle: the call allocates nothing and can be captured in a graph.
 *     0 for T < 4, for BSRNN / FSPEN / LiSenNet and for a null handle: work_dev may then be NULL.
 *   Dispatch: the width of the pipeline is fe_spec_step's (T >= 4, at most half as many streams as CUs, fe_set_time_pipeline not 0 or 1),
 *     and the chunk must cover the overlap: T * H >= N - H.  T >= 4 gives that for every shipped shape except hop 100 / n_fft 512
 *     (FastEnhancer_L, dprnn L) and hop 200 / n_fft 1024 (48 kHz L), where N - H = 4.12 H: those need T >= 5.
 *     Where that is 0 - and for BSRNN, FSPEN and LiSenNet, whose streaming steps are not pipelined - the call makes the very launch fe_step
 *     makes: bit-identical results.  A cooperative launch the runtime refuses falls back to the same walk.
 *   Two launches: the pipelined frame kernel, whose frames read the call's cache_stft / wav_in and store their windowed output to work_dev,
 *     then stream_ola_kernel - the streaming overlap-add (old cache_istft, then the covering frames, oldest first) and the two new STFT
 *     caches.  fe_last_step_kernel: "fe_frame_kernel<time-pipelined, streaming> + stream_ola_kernel [shape B]".
 *   BSRNN and FSPEN chunks on the time pipeline: fe_step_backlog, below. */
size_t fe_step_chunk_work_floats(const fe_handle* h, int B, int T);
int fe_step_chunk(fe_handle* h, const float* wav_in_dev, size_t in_stride, float* state_dev, float* wav_out_dev, size_t out_stride,
                  int B, int T, float* work_dev, void* stream);

/* fe_step for few streams and many hops, for EVERY family with a streaming state: fe_step(h, ..., B, T, stream) with the T frames of each
 * stream on the time pipeline wherever the family has one.  Rows, state buffer (fe_state_floats(h, B), updated in place), argument checks
 * (before the handle's weights), error codes and refusals are fe_step's, as for fe_step_chunk; the noncausal model is refused with
 * fe_step's message.
 *   FastEnhancer family (default, ln, dprnn, time_kernel, dptransformer): the call IS fe_step_chunk and the query IS
 *     fe_step_chunk_work_floats - everything above holds word for word.
 *   BSRNN and FSPEN: the T frames of each stream run on P co-resident workgroups - the family's time-pipelined frame kernel, the one of
 *     its fe_offline, in streaming mode - which exchange only the time-LSTM (h, c) per layer (BSRNN) or the inter-GRU states per DPE block
 *     (FSPEN), in place in the caller's state: frame 0 reads it, the last frame leaves the new one.  Every frame reads the call's old
 *     cache_stft and wav_in and stores its windowed output to work_dev; stream_ola_kernel then does the streaming overlap-add and writes
 *     both STFT caches.
 *     Results: wav_out and every model-state tensor agree with fe_step(B, T) to fp32 rounding (the overlap-add sums are formed in another
 *       order); cache_stft agrees bit for bit.  The state left behind is valid for every other entry point: fe_step, the export and
 *       import records, a later fe_step_backlog.
 *     work_dev: fe_step_backlog_work_floats(h, B, T) floats - the frame counters [B][layers or blocks], rounded up to 4 floats, then the
 *       windowed frames [B][T][N].  The size depends on the model, B and T only and is monotone in both; 0 for T < 4, for B <= 0 and for a
 *       null handle, non-zero for every B >= 1 and T >= 4 whatever fe_set_time_pipeline says: a buffer sized once serves every setting.
 *       NULL where the pipelined path would run is FE_ERR_INVALID_ARG.
 *     Width P: that of the family's pipelined fe_offline (fe_set_time_pipeline; BSRNN up to 64, FSPEN up to 32 frames in flight, at most
 *       the co-resident workgroups the B streams leave each other), and the chunk must cover the overlap, T * H >= N - H (every shipped
 *       BSRNN and FSPEN shape does at T = 4).  P = 0 - T < 4, fe_set_time_pipeline(0 or 1), too many streams to give each two workgroups -
 *       and a cooperative launch the runtime refuses: the call makes the very launch fe_step makes, bit for bit.
 *     A linear chain of three kernels on the caller's stream (the counters are zeroed by a small kernel, not a memset node); the call
 *       allocates nothing and can be captured into a graph.  wav_in and wav_out MUST NOT overlap, as for fe_step_chunk.
 *     fe_last_step_kernel: "bsrnn_frame_kernel<time-pipelined, streaming> + stream_ola_kernel [shape xxt]",
 *       "fspen_frame_kernel<time-pipelined, streaming> + stream_ola_kernel [shape fspen]" (the counters' zeroing is not named).
 *   LiSenNet: at the default setting, and under fe_set_time_pipeline(0 or 1), the call is fe_step's launch, and
 *     fe_step_backlog_work_floats is 0 at every setting.  The pipeline is OPT-IN by an explicit width: under fe_set_time_pipeline(P) with
 *     P >= 2, with T >= 4, T * H >= N - H and a work_dev of fe_lisennet_backlog_work_floats(h, B, T) floats, the T frames of each stream
 *     run on the family's time-pipelined frame kernel in its streaming instantiation.  That kernel hands NINE caches from frame to frame
 *     (the phase, three encoder frames, per block the GRU state and the ConvGLU's two frames, the decoder frame) through ring slots in
 *     work_dev; frame 0 takes each from the caller's state, the last frame (the ConvGLU: the last two) leaves its own there, in place.
 *     Results, the chain of three kernels, graph capture and the no-overlap rule are as for BSRNN and FSPEN above.
 *     fe_last_step_kernel: "lisennet_frame_kernel<time-pipelined, streaming> + stream_ola_kernel [shape lisennet]".
 *     work_dev == NULL, T < 4 and a cooperative launch the runtime refuses: fe_step's launch, bit for bit (NULL is not an error here).
 *     fe_lisennet_backlog_work_floats(h, B, T): the frame counters [B][9] rounded up to 4 floats, the windowed frames [B][T][N] and the
 *       rings [B][66][cache floats of a stream] (sized for the widest pipeline, as fe_offline_work_floats sizes them) - whatever
 *       fe_set_time_pipeline says; 0 for every other family, for B <= 0, for T < 4 and for a null handle. */
size_t fe_step_backlog_work_floats(const fe_handle* h, int B, int T);
int fe_step_backlog(fe_handle* h, const float* wav_in_dev, size_t in_stride, float* state_dev, float* wav_out_dev, size_t out_stride,
                    int B, int T, float* work_dev, void* stream);
size_t fe_lisennet_backlog_work_floats(const fe_handle* h, int B, int T);

/* The packet step's time-pipelined form - a stream of a packet batch that comes back with a backlog: fe_step_streams_banked[_pinned] with the
 * hops of EACH stream spread over co-resident workgroups instead of walked by one.  Same descriptors, slots, formats, limit, meters and banks,
 * in place on the capacity-sized state buffer.
 *   Meaning: for every stream of the call, what fe_step_streams_banked[_pinned] gives for the same arguments.  Unchanged: the kernel reads the
 *     descriptors when it runs; hops is clamped to [0, T_max]; a stream whose input or output range leaves [0, count) is skipped like a 0-hop
 *     stream (checked in the kernel, on both sides); a slot outside [0, capacity) or a bank outside [0, n_banks) gives zero output rows, no
 *     state write and no level row; min_gain, levels and bank may each be NULL; FE_ERR_NO_WEIGHTS unless every bank is loaded when
 *     bank != NULL; the int16 conversion rules; the host checks, all before any device work.  BSRNN, FSPEN, LiSenNet and the noncausal model
 *     are refused as fe_step_streams refuses them.
 *   Results: output samples and every state tensor of the named slots agree with the serial packet step to fp32 rounding (the frames' sums
 *     are formed in another order); cache_stft, a copy of input samples, bit for bit; every float of state_dev that belongs to a slot the
 *     call does not advance is left bit for bit.  Level rows: in_peak is exact, the other three words agree to rounding; a row is formed
 *     without atomics in a fixed order - bitwise reproducible from run to run at a fixed pipeline width.
 *   Any hop count 0 .. T_max of a stream is served on the pipeline (the host cannot see the descriptors), 1, 2, 3 hops and
 *     hops * H < N - H included: the audio kernel orders every read of a stream's old STFT caches before every write of its new ones.
 *   wav_in and wav_out MUST NOT overlap, as for fe_step_chunk.
 *   work_dev: fe_step_streams_chunk_work_floats(h, n, T_max) floats - frame counters and the windowed frames [n][T_max][N].  The size depends on
 *     the model, n and T_max only and is monotone in both.  0 where the call never pipelines (T_max < 4, the ring variants, the baseline
 *     families, a null handle): work_dev may then be NULL.  The call allocates nothing and may be captured into a graph: a linear chain of
 *     three kernels (the counters are zeroed by a small kernel: a captured memset node of their odd byte count did not replay reliably).
 *   It does not pipeline - and then IS fe_step_streams_banked[_pinned] with the same arguments, bit for bit, which fe_last_step_kernel shows -
 *     when the pipeline's width is 0 (T_max < 4, 2 n > #CUs, fe_set_time_pipeline(0 or 1)); for the ring variants (time_kernel,
 *     dptransformer: the kernels that move their rings are not slotted); when the runtime refuses the cooperative launch.
 *   fe_last_step_kernel on the pipelined path: "fe_frame_kernel<time-pipelined, streams[, pinned][, s16][, banks]> + stream_ola_streams_kernel"
 *     (the counters' zeroing is not named). */
size_t fe_step_streams_chunk_work_floats(const fe_handle* h, int n, int T_max);
int fe_step_streams_chunk(fe_handle* h, const void* wav_in_dev, size_t in_count, float* state_dev, int capacity, const fe_stream_desc* desc_dev,
                          void* wav_out_dev, size_t out_count, int n, int T_max, int format, const float* min_gain, fe_stream_levels* levels,
                          const int* bank, float* work_dev, void* stream);
int fe_step_streams_chunk_pinned(fe_handle* h, const void* wav_in_host, size_t in_count, float* state_dev, int capacity,
                                 const fe_stream_desc* desc_dev, void* wav_out_host, size_t out_count, int n, int T_max, int format,
                                 const float* min_gain, fe_stream_levels* levels, const int* bank, float* work_dev, void* stream);

/* The packet step's time-pipelined form for EVERY family with a streaming state: fe_step_pool_streams_ctl[_pinned] with the hops of EACH
 * stream spread over co-resident workgroups instead of walked by one - to fe_step_pool_streams_ctl what fe_step_streams_chunk is to
 * fe_step_streams_banked.  Same descriptors, slots, formats, limit and meters, in place on the capacity-sized state buffer.
 *   Meaning: for every stream of the call, what fe_step_pool_streams_ctl[_pinned] gives for the same arguments - the kernel reads the
 *     descriptors when it runs; hops is clamped to [0, T_max]; a stream whose input or output range leaves [0, count) is skipped like a 0-hop
 *     stream (checked in the kernel, by every workgroup of the stream and by the audio kernel); a slot outside [0, capacity) gives zero output
 *     rows, no state write and no level row; min_gain and levels may each be NULL; the int16 conversion rules.
 *   FastEnhancer family: the call IS fe_step_streams_chunk[_pinned] with bank = NULL and the query IS fe_step_streams_chunk_work_floats - the
 *     same launch, the same bits, the same refusals; the noncausal model is refused with fe_step's message.  (fe_step_streams_chunk itself
 *     keeps refusing BSRNN, FSPEN and LiSenNet.)
 *   BSRNN and FSPEN: the hops of each stream run on P co-resident workgroups - the time-pipelined PACKET instantiation of the family's frame
 *     kernel: workgroup p of a stream runs its frames p, p + P, ... < hops, the frames exchange only the time-LSTM (h, c) per layer (BSRNN) or
 *     the inter-GRU states per DPE block (FSPEN), in place at the stream's slot of the caller's state; every frame reads the slot's old
 *     cache_stft and the stream's samples, applies the stream's limit in the compressed domain and stores its windowed output to work_dev.
 *     stream_ola_streams_kernel then does each stream's streaming overlap-add, writes its output rows (zero rows for a stream without state),
 *     both STFT caches and its level row.
 *     Host checks: those of fe_step_pool_streams_ctl[_pinned] - the same codes, the same wording under this function's name - all before any
 *       device work, the argument checks before the weights check.  work_dev == NULL where the pipeline would run is FE_ERR_INVALID_ARG (an
 *       argument check; the message names the query).  The two tables are looked up as fe_step_pool_streams_ctl looks them up.
 *     Results: output samples and every model-state tensor of the stepped slots agree with fe_step_pool_streams_ctl to fp32 rounding (the
 *       frames' sums are formed in another order); cache_stft, a copy of input samples, bit for bit; every float of state_dev that belongs to
 *       a slot the call does not advance keeps its bits; no sample outside the rows the descriptors name is written.  Level rows: in_peak is
 *       exact, the other three words agree to rounding; a row is formed without atomics in a fixed order - bitwise reproducible from run to
 *       run at a fixed pipeline width.  The limit touches the output path only: every state tensor but cache_istft holds the bits of the
 *       unlimited pipelined run.
 *     Any hop count 0 .. T_max of a stream is served on the pipeline (the host cannot see the descriptors), 1, 2, 3 hops included: there is
 *       no T * H >= N - H condition - the audio kernel orders every read of a stream's old STFT caches before every write of its new ones.
 *     work_dev: fe_step_pool_streams_chunk_work_floats(h, n, T_max) floats - the frame counters [n][layers or blocks], rounded up to 4 floats,
 *       then the windowed frames [n][T_max][N] (fe_step_backlog's layout).  The size depends on the model, n and T_max only and is monotone in
 *       both; 0 for T_max < 4, for n <= 0 and for a null handle, non-zero for every n >= 1 and T_max >= 4 whatever fe_set_time_pipeline
 *       says: a buffer sized once serves every setting.
 *     Width P: that of the family's pipelined fe_offline for n streams of T_max frames (fe_set_time_pipeline; at most the co-resident
 *       workgroups the n streams leave each other).  P = 0 - T_max < 4, fe_set_time_pipeline(0 or 1), too many streams to give each two
 *       co-resident workgroups - and a cooperative launch the runtime refuses: the call makes the very launch of
 *       fe_step_pool_streams_ctl[_pinned], bit for bit, which fe_last_step_kernel shows.
 *     A linear chain of three kernels on the caller's stream (the counters are zeroed by a small kernel, not a memset node); the call
 *       allocates nothing and can be captured into a graph.  wav_in and wav_out MUST NOT overlap.
 *     fe_last_step_kernel on the pipelined path: "bsrnn_frame_kernel<time-pipelined, streams[, pinned][, s16]> + stream_ola_streams_kernel
 *       [shape xxt]", "fspen_frame_kernel<time-pipelined, streams[, pinned][, s16]> + stream_ola_streams_kernel [shape fspen]" (the counters'
 *       zeroing is not named).
 *   LiSenNet: at the default setting, and under fe_set_time_pipeline(0 or 1), the call is fe_step_pool_streams_ctl[_pinned]'s launch, bit
 *     for bit and under that name, and fe_step_pool_streams_chunk_work_floats is 0 at every setting.  The pipeline is OPT-IN, on
 *     fe_step_backlog's terms: under an explicit fe_set_time_pipeline(P) with P >= 2, with T_max >= 4, a width of at least two workgroups
 *     per stream for n streams and a work_dev of fe_lisennet_pool_streams_chunk_work_floats(h, n, T_max) floats, the hops of each stream
 *     run on the time-pipelined PACKET instantiation of the family's frame kernel.  Its frames hand the NINE caches on through ring slots
 *     in work_dev; frame 0 takes each from the stream's slot of the caller's state, the stream's last frame (the ConvGLU: its last two;
 *     a one-hop stream: the one frame, which also moves the newer half to the older) leaves its own there, in place.  Any hop count
 *     0 .. T_max is served there.  Meaning, results, the chain of three kernels, graph capture and the no-overlap rule are as for BSRNN and
 *     FSPEN above.
 *     fe_last_step_kernel: "lisennet_frame_kernel<time-pipelined, streams[, pinned][, s16]> + stream_ola_streams_kernel [shape lisennet]".
 *     work_dev == NULL (not an error for this family), T_max < 4, too many streams to give each two co-resident workgroups and a cooperative
 *     launch the runtime refuses (by then only the counters in work_dev have been written): the launch of fe_step_pool_streams_ctl[_pinned].
 *     The argument checks and their order are those of every family.
 *     fe_lisennet_pool_streams_chunk_work_floats(h, n, T_max): the frame counters [n][9] rounded up to 4 floats, the windowed frames
 *       [n][T_max][N] and the rings [n][66][cache floats of a stream] (sized for the widest pipeline) - whatever fe_set_time_pipeline
 *       says; monotone in n and T_max; 0 for every other family, for n <= 0, for T_max < 4 and for a null handle. */
size_t fe_step_pool_streams_chunk_work_floats(const fe_handle* h, int n, int T_max);
size_t fe_lisennet_pool_streams_chunk_work_floats(const fe_handle* h, int n, int T_max);
int fe_step_pool_streams_chunk(fe_handle* h, const void* wav_in_dev, size_t in_count, float* state_dev, int capacity, const fe_stream_desc* desc_dev,
                               void* wav_out_dev, size_t out_count, int n, int T_max, int format, const float* min_gain, fe_stream_levels* levels,
                               float* work_dev, void* stream);
int fe_step_pool_streams_chunk_pinned(fe_handle* h, const void* wav_in_host, size_t in_count, float* state_dev, int capacity,
                                      const fe_stream_desc* desc_dev, void* wav_out_host, size_t out_count, int n, int T_max, int format,
                                      const float* min_gain, fe_stream_levels* levels, float* work_dev, void* stream);

/* Engine of fe_offline for the default and noncausal FastEnhancer models:
 *   FE_OFFLINE_TIME_BATCHED (the default where compiled; the only engine of the noncausal model): the network is cut at the
 *     blocks' time GRUs and every piece runs over ALL frames of ALL utterances, layer by layer, as the reference's own offline
 *     forward does (model.py:620-675): encoder pass (tiles of frames as one GEMM per layer), per block a scan over time in
 *     which only W_hh h is serial (the x half of the gates is batched) + a batched attention pass, decoder pass, overlap-add
 *     (csrc/tb_kernels.hip.h).  Activations that cross a GRU live in work_dev.
 *     With few utterances the scan runs four rows per workgroup on v_mfma_f32_4x4x1 instead of sixteen on 16x16x4.
 *   FE_OFFLINE_FRAME_WALK: the per-hop kernel walking (or, fe_set_time_pipeline, pipelining) the frames of each utterance.
 *   FE_OFFLINE_AUTO: time-batched, except for the big shapes (rf_channels >= 72) with 8 or more utterances, where the pipelined
 *     walk of the per-hop kernel is the faster one.
 * fe_spec_step follows the same setting: FE_OFFLINE_TIME_BATCHED runs every chunk of T >= 2 frames on the time-batched engine (the
 * scans start from the caller's GRU caches and leave the new ones), AUTO the chunks of 16+ frames of batches too large for the time
 * pipeline (or of 2048+ frames in all); the handle then keeps a grow-only work buffer (a first / larger call allocates).
 * Results agree to fp32 rounding.  The other architectures / variants always walk.  A handle's compute calls must be stream-ordered
 * (one stream, or event-ordered streams): the engines keep per-handle scratch, counters and helper streams. */
/* Which kernel runs the per-hop streaming step (fe_step / fe_step_host with T = 1) of the default FastEnhancer model:
 *   FE_STEP_KERNEL_WAVES4: one 256-thread workgroup per stream (fe_kernels.hip.h), the kernel every other entry point uses too;
 *   FE_STEP_KERNEL_WG8 (default): where built for the shape (FastEnhancer_B), one 512-thread workgroup per stream - two waves per
 *     SIMD, GRU gates grouped by channel (fe_frame8.hip.h) - for batches of up to one stream per CU;
 *   FE_STEP_KERNEL_WG8_PERSIST: the same also above that (persistent workgroups instead of the low-LDS companion kernel).
 * The two kernels agree to fp32 rounding (a few 1e-8 on the waveform), not bit for bit: a caller that needs a chunked launch
 * (T > 1) to be bit-identical to T per-hop launches selects FE_STEP_KERNEL_WAVES4.  The environment variable FE_WG8 = 0 | 1 | 2
 * sets the value new handles start with (any other value is ignored).  The reference has one forward only (models/fastenhancer/default/model.py:677-710).
 * BSRNN with num_channels = 16 (r5): FE_STEP_KERNEL_WAVES4 runs the layers of the per-hop step phase by phase on all four waves
 * (bsrnn_frame_kernel<PART 1>), any other value the role-split kernel (bsrnn_ov_kernels.hip.h) for batches of up to one stream per CU;
 * the two agree to fp32 rounding.  (models/bsrnn/model.py:367-390) */
#define FE_STEP_KERNEL_WAVES4 0
#define FE_STEP_KERNEL_WG8 1
#define FE_STEP_KERNEL_WG8_PERSIST 2
int fe_set_step_kernel(fe_handle* h, int kernel);

/* The other kernel-selection switches of a handle, by name (r6; until r5 these were environment variables read in three files).
 * FE_ERR_INVALID_ARG for an unknown name or a value outside the option's range; fe_options() / fe_option_name(i) enumerate them.
 *   name                       range      default  meaning
 *   "bsrnn_role_split"         0 | 1      1        BSRNN, num_channels 16, up to one stream per CU: PART 1 of the per-hop step on the role-split
 *                                                  kernel (bsrnn_ov_kernels.hip.h); 0 = the phase-by-phase kernel (what fe_set_step_kernel(WAVES4) selects too)
 *   "bsrnn_stream_batch_min"   0 .. 2^24  2048     BSRNN, num_channels 16 and (r6) 32: from this many streams the layers run batched over the streams
 *                                                  (bsrnn_sb_kernels.hip.h); 0 = never
 *   "bsrnn_three_launch_step"  0 | 1      1        BSRNN per-hop step as PART 1 -> batched mask decoder -> PART 2; 0 = one fused kernel per stream
 *   "bsrnn_ov_profile"         0 | 1      0        fe_profile_step probes the role-split PART 1 instead of the fused kernel's phases
 *   "fspen_stream_batch_min"   0 .. 2^24  1536     FSPEN: from this many streams the middle of the network runs batched over the streams; 0 = never
 *   "low_lds_companion"        0 | 1      1        FastEnhancer per-hop step above the streams the shape's own LDS plan holds at once (one per CU; two for
 *                                                  FastEnhancer_T): the low-LDS companion kernel (two workgroups per CU, three for the T shapes) where one
 *                                                  is compiled; 0 = persistent workgroups of the shape's own kernel
 *   "bsrnn_fused_step"         0 | 1      0        BSRNN, num_channels 16, up to one stream per CU (r6): the whole per-hop step in ONE cooperative launch -
 *                                                  the workgroups of a sixteen-stream tile meet at a barrier after the layers, run the mask decoder for
 *                                                  their tile, meet again and finish their own streams; 0 = three launches (a launch the runtime
 *                                                  refuses falls back to them by itself).  Bit-identical results; MEASURED SLOWER (barriers across XCDs,
 *                                                  cooperative launch: profiles/r6_bsrnn_fused_step.txt), hence off by default
 *   "lisennet_stream_batch_min" 0 .. 2^24 513      LiSenNet (r6): from this many streams the per-hop step runs encoder.conv_1 .. the mask head batched over the streams on
 *                                                  the matrix cores (lisennet_sb_kernels.hip.h: STFT + features per stream, sixteen streams per workgroup, mask + iSTFT per stream); 0 = never
 * A/B scripts (tools/ab_*.sh) preset the values NEW handles start with through FE_BSRNN_OV, FE_BSRNN_SB, FE_BSRNN_SPLIT, FE_BSRNN_OV_PROF,
 * FE_FSPEN_SB, FE_LOWLDS (FE_NO_LOWLDS), FE_BSRNN_FUSED, FE_LISENNET_SB and FE_WG8 (the step kernel): read once, in fe_create, validated against the same ranges (anything else
 * is ignored).  The reference has one forward per model and nothing to select (models/fastenhancer/default/model.py:677-710). */
int fe_set_option(fe_handle* h, const char* name, int value);
int fe_get_option(const fe_handle* h, const char* name, int* value);
int fe_options(void);
const char* fe_option_name(int idx);

/* What the handle's last compute call (fe_step / fe_step_host / fe_spec_step / fe_offline / fe_offline_ragged / fe_debug_step / fe_profile_step)
 * enqueued: the kernel family and instantiation of every launch in order, as the launchers name them, " + "-joined, repeats as "n x", then the
 * compiled shape record - e.g. "fe_frame8_kernel [shape B]", "fe_frame_kernel<LOW=2, per-hop> [shape B48H480LOW]",
 * "bsrnn_ov_kernel + bsrnn_mlp_kernel<one 16-stream tile per workgroup> + bsrnn_frame_kernel<PART 2> [shape xt]".  These are the names
 * rocprofv3 --kernel-trace shows (bench.py's roofline.kernel is this string).  "" before the first call.  The pointer is valid until the
 * next call of this function on the handle. */
const char* fe_last_step_kernel(const fe_handle* h);

#define FE_OFFLINE_AUTO 0
#define FE_OFFLINE_FRAME_WALK 1
#define FE_OFFLINE_TIME_BATCHED 2
int fe_set_offline_engine(fe_handle* h, int engine);

/* Offline wav->wav, Model.forward (model.py:728-735) with CompressedSTFT
 * (functional/audio_modules.py:70-164): noisy [B, Tw] -> wav_hat [B, H*(Tw/H)], spec_hat [B, N/2, T, 2],
 * T = 1 + Tw/H.  work_dev: scratch of fe_offline_work_floats(B, Tw) floats.
 * The size is that of the engine the CURRENT fe_set_offline_engine / fe_set_time_pipeline setting selects and is monotone in B and Tw
 * under that setting: a buffer sized once for the largest batch serves every smaller one (AUTO on the big shapes covers both the frame
 * walk of 8+ utterances and the time-batched pass of fewer).  After fe_set_offline_engine the size must be queried again - the
 * time-batched engine of FastEnhancer_L needs ~100x the frame walk's scratch, and fe_offline cannot see the size of work_dev. */
size_t fe_offline_work_floats(const fe_handle* h, int B, int Tw);
int fe_offline(fe_handle* h, const float* noisy_dev, int B, int Tw, float* wav_hat_dev,
               float* spec_hat_dev, float* work_dev, void* stream);

/* The same for a batch of utterances of DIFFERENT lengths - what the reference's offline caller does file by file
 * (scripts/test_pytorch.py:28-37: one Model.forward per file of the directory): utterance b = noisy_dev[b * in_stride + n],
 * n < Tw_host[b] (a HOST array, read before the call returns); wav_hat_dev[b * out_stride + n], n < H * (Tw[b] / H), the rest of a row is
 * left untouched; spec_hat_dev [B, F, Tmax, 2] with Tmax = 1 + max(Tw) / H (F = N/2 for FastEnhancer), the frames of an utterance past
 * its own 1 + Tw[b] / H unspecified.  On the time-batched engine (the default FastEnhancer model and the noncausal one) this is ONE
 * batched pass laid out for the longest utterance - every utterance's result is bit-identical to its own fe_offline call on that engine
 * (frames are rows of the layer GEMMs, scans are per row; the reflect padding, the reverse scans of the noncausal model and the
 * overlap-add use each utterance's own length); sort a directory by length to keep the padding small.  A ragged batch takes that pass
 * under FE_OFFLINE_AUTO too, whatever the shape and B (the frame walk AUTO prefers for 8+ equal-length utterances of the big shapes has
 * no ragged form).  The other models / variants and FE_OFFLINE_FRAME_WALK have no batched form (one length per launch): the call runs
 * them one utterance after the other, each on the engine fe_offline would take for a single utterance.
 * work_dev: fe_offline_ragged_work_floats(B, max(Tw)) floats (same contract as fe_offline_work_floats: query again after
 * fe_set_offline_engine). */
size_t fe_offline_ragged_work_floats(const fe_handle* h, int B, int Tw_max);
int fe_offline_ragged(fe_handle* h, const float* noisy_dev, size_t in_stride, const int* Tw_host, int B, float* wav_hat_dev, size_t out_stride,
                      float* spec_hat_dev, float* work_dev, void* stream);

/* The STFT front / back ends as launches of their own - the modules the reference exposes as `model.stft` and that
 * scripts/export_onnx.py:55-57 composes line by line (inside fe_step / fe_offline they are fused into the frame kernel).
 * No weights needed.  Streaming, one hop (ONNXSTFT.forward / .inverse, functional/audio_modules.py:243-303):
 *   fe_stft_step : wav_in [b*in_stride + n] (n < H), cache_in [B, N-H] -> spec [B, N/2+1, 1, 2], cache_out [B, N-H]
 *   fe_istft_step: spec [B, N/2+1, 1, 2], cache_in [B, N-H] -> wav_out [b*out_stride + n] (n < H), cache_out [B, N-H]
 * Functional like the reference: cache_in is not modified unless cache_out aliases it. */
int fe_stft_step(fe_handle* h, const float* wav_in_dev, size_t in_stride, const float* cache_in_dev, float* cache_out_dev,
                 float* spec_out_dev, int B, void* stream);
int fe_istft_step(fe_handle* h, const float* spec_in_dev, const float* cache_in_dev, float* cache_out_dev,
                  float* wav_out_dev, size_t out_stride, int B, void* stream);
/* Offline, centered (CompressedSTFT.forward / .inverse, functional/audio_modules.py:124-164 over STFT :70-119), one
 * workgroup per (stream, frame):
 *   fe_stft_offline : noisy [B, Tw] -> spec [B, F, T, 2], T = 1 + Tw/H; F = N/2 (discard_last_freq_bin) or N/2+1;
 *                     compress != 0: X *= max(|X|, 1e-5)^(c-1) with c = input_compression
 *   fe_istft_offline: spec [B, F, T, 2] (complex) -> wav [B, H*(T-1)]; compress != 0: X *= |X|^(1/c-1) first;
 *                     frames_dev: scratch of B*T*N floats */
int fe_stft_offline(fe_handle* h, const float* noisy_dev, int B, int Tw, int F, int compress, float* spec_out_dev, void* stream);
int fe_istft_offline(fe_handle* h, const float* spec_in_dev, int B, int T, int F, int compress, float* wav_out_dev,
                     float* frames_dev, void* stream);

/* Analytic FLOPs of one frame (2*MACs of models/fastenhancer/default/macs.py:17-87 + FFTs). */
double fe_flops_per_frame(const fe_handle* h);

/* Debug: run ONE hop (T=1) and dump the named per-stage activations of every stream to dbg_dev.
 * fe_debug_stages() reports name / rows / cols / offset of each dump ([rows][cols] row-major per
 * stream, stream-major). Used by the parity tests to localise a mismatch. */
int fe_debug_stages(const fe_handle* h);
int fe_debug_stage(const fe_handle* h, int idx, const char** name, int* rows, int* cols, size_t* offset_floats);
size_t fe_debug_floats(const fe_handle* h);   /* per stream */
int fe_debug_step(fe_handle* h, const float* wav_in_dev, size_t in_stride, float* state_dev,
                  float* wav_out_dev, size_t out_stride, int B, float* dbg_dev, void* stream);

/* Profiling: like fe_step, and thread 0 of workgroup 0 stores the shader cycle counter (s_memtime) at
 * the phase boundaries of the LAST frame into clk_dev[0..63] (see fe_kernels.hip.h, FE_CLK; BSRNN:
 * bsrnn_kernels.hip.h, BE_CLK).  Runs the debug / profile instantiation of the kernel, not the one fe_step runs;
 * tools/gpu_phases.py and tools/gpu_phases_bsrnn.py print the table. */
int fe_profile_step(fe_handle* h, const float* wav_in_dev, size_t in_stride, float* state_dev,
                    float* wav_out_dev, size_t out_stride, int B, int T, unsigned long long* clk_dev, void* stream);

/* Test support (r5): fills the LDS of every CU of the current device with NaN bit patterns (a short launch on `stream`).  The kernels
 * read padded operands in places - zero weights against words past the end of a tensor in LDS - and whatever an earlier kernel left
 * there must not matter: the parity tests run a step after this call and require the bits of the un-poisoned run.
 * (The reference has no counterpart: PyTorch pads explicitly, models/bsrnn/model.py:136-153.) */
int fe_debug_poison_lds(void* stream);

/* Test support: the packing fe_load_weights does between its two copies, host to host - no HIP call, works without a GPU (as fe_create
 * does).  blob_host: the fused blob (nfloats == fe_weight_floats(h)); out_host: the buffer the kernels read, *packed_floats its size.
 * out_host == NULL reports the size only.  A null handle or blob, a wrong nfloats or a capacity below the packed size is
 * FE_ERR_INVALID_ARG with nothing written. */
int fe_debug_pack_weights(fe_handle* h, const float* blob_host, size_t nfloats, float* out_host, size_t capacity, size_t* packed_floats);

/* ---- Audio at another sample rate: a polyphase resampler sr_in -> sr_out, for whole signals and for packet streams.
 * (The reference's callers load every file with librosa.load(path, sr=model_rate) - scripts/test_onnx.py:14, scripts/test_pytorch.py:29 - and
 * scripts/resample.py:75-80 offers this filter as its `polyphase` type: scipy.signal.resample_poly(x, up, down) with its defaults.)
 *
 * The contract.  g = gcd(sr_in, sr_out), up = sr_out / g, down = sr_in / g, R = max(up, down), hl = 10 R, L = 2 hl + 1.
 * Taps h[t] = up * h0[t], h0[t] = sinc((t - hl) / R) / R * I0(5 sqrt(1 - ((t - hl) / hl)^2)) / I0(5) scaled to sum 1 - that is
 * up * firwin(L, 1 / R, window = ("kaiser", 5.0)) - designed in double and rounded to fp32 once.  K = ceil(L / up) taps per output.
 * Output m of an input x[0 .. N):  c = m down + hl,  kmax = c div up,  r = c mod up,
 *     y[m] = sum over j = 0 .. K - 1 with r + j up <= 2 hl of  h[r + j up] * x[kmax - j],      x = 0 outside [0, N),
 * accumulated in fp32 from +0 with j ascending, one fused multiply-add per tap.  Against the same sum in double the error is at most
 * (K + 2) 2^-24 S max|x| with S = max over r of sum over j of |h[r + j up]| (a K-term fp32 dot product and one rounding of each tap).
 * A whole-signal call returns ceil(N up / down) outputs.  A stream that has consumed N samples has emitted
 *     M(N) = max(0, ceil((N up - hl) / down))
 * outputs - every output whose newest input x[kmax] has arrived - so its latency is hl / up input samples (30 at 48 -> 16 kHz, 10 at
 * 8 -> 16 kHz), and under ANY packetisation its outputs are the first M(N) outputs of the whole-signal call on the same samples, bit for
 * bit.  There is no flush: a caller that wants the tail pushes hl / up zeros.  int16 input is the float input s / 32768 (exact); int16
 * output is clamp(rint(y * 32768), -32768, 32767), ties to even, NaN -> 0, of the float output (the rules of fe_step_streams).
 *
 * G.711 (FE_AUDIO_ULAW, FE_AUDIO_ALAW: telephony's one byte per sample, RTP payload types 0 and 8).  fe_resample, fe_resample_streams[_pinned]
 * and fe_resample_rings[_pinned] take them as in_format and as out_format, independently (mu-law in and float out, int16 in and A-law out).
 * Every count, stride, offset and ring base / length / position stays in ELEMENTS of the format - bytes here - and any byte alignment is
 * legal.  All arithmetic below is on 32-bit ints, >> is arithmetic, hibit(v) is the index of the highest set bit.
 *   In: a byte b is the 16-bit linear sample s = dec(b), seen as the float s / 32768 exactly as an int16 s is.
 *     mu-law: u = ~b & 0xFF, e = (u >> 4) & 7, m = u & 15, mag = (((m << 3) + 0x84) << e) - 0x84, s = (u & 0x80) ? -mag : mag
 *             (-32124 .. 32124; 0xFF and 0x7F both decode to 0)
 *     A-law:  a = b ^ 0x55, e = (a >> 4) & 7, m = a & 15, mag = e == 0 ? (m << 4) + 8 : ((m << 4) + 0x108) << (e - 1),
 *             s = (a & 0x80) ? mag : -mag       (-32256 .. 32256)
 *   Out: the float y is quantised by the int16 rule above to q, then b = enc(q).
 *     mu-law: v = q >> 2; if v < 0: mask = 0x7F, v = -v, else mask = 0xFF; v = min(v, 8159) + 33, seg = hibit(v) - 5,
 *             t = seg >= 8 ? 0x7F : (seg << 4) | ((v >> (seg + 1)) & 15), b = t ^ mask
 *     A-law:  if q >= 0: n = q, sign = 0x80, else n = ~q, sign = 0; if n < 256: e = 0, m = n >> 4, else e = hibit(n) - 7,
 *             m = (n >> (e + 3)) & 15; b = (sign | (e << 4) | m) ^ 0x55
 *   These are the ITU-T G.711 tables as CPython's audioop computes them (ulaw2lin, alaw2lin, lin2ulaw, lin2alaw on 16-bit samples).
 * The state row is floats whatever the formats: a row written under one input format continues under another.  Streaming exactness is
 * unchanged: under any packetisation the output bytes are the first M(N) bytes of the whole-signal call.  "Nothing outside a stream's
 * ranges is written" holds to the BYTE: no store covers a byte that is not the stream's.  A call with a G.711 format on either side runs
 * an instantiation of its own, and fe_resampler_last_kernel names it with g711 as the last item: fe_resample_kernel<whole,g711>,
 * <streams,g711>, <streams,pinned,g711>, <ring,g711>, <ring,pinned,g711>; every other call runs and reports what it did before.
 * Not here: G.711 straight into a model step (fe_step_streams* and fe_step_pool_streams* refuse the two codes), G.711 WAV files, G.722
 * and other codecs.
 *
 * The create call and every query work without a GPU (as the model handle's do); the tap table is uploaded to the device that is current
 * at the handle's FIRST launch (one allocation and one synchronous copy: make that launch outside a graph capture), and the handle
 * belongs to that device from then on.  Equal rates or a rate <= 0 are FE_ERR_INVALID_ARG; a reduced ratio with max(up, down) > 640 is
 * FE_ERR_UNSUPPORTED_CONFIG (every pair among 8, 11.025, 12, 16, 22.05, 24, 32, 44.1 and 48 kHz fits - 48 -> 11.025 kHz is 147 / 640 -
 * except 11.025 <-> 32 kHz, which is 441 / 1280). */
typedef struct fe_resampler fe_resampler;
int fe_resampler_create(int sr_in, int sr_out, fe_resampler** out);
void fe_resampler_destroy(fe_resampler* rs);
int fe_resampler_up(const fe_resampler* rs);
int fe_resampler_down(const fe_resampler* rs);
int fe_resampler_taps_per_output(const fe_resampler* rs);      /* K */
int fe_resampler_half_len(const fe_resampler* rs);             /* hl */
/* the L = 2 hl + 1 taps h in double, as designed (n < L is FE_ERR_INVALID_ARG with nothing written; out == NULL returns L) */
int fe_resampler_taps(const fe_resampler* rs, double* out, size_t n);
/* ceil(n_in up / down); and M(consumed + n_in) - M(consumed), what a stream emits for its next n_in samples.  Negative arguments give -1. */
long long fe_resampler_out_count(const fe_resampler* rs, long long n_in);
long long fe_resampler_produced(const fe_resampler* rs, long long consumed, long long n_in);
/* floats of one stream's state row (below) */
size_t fe_resampler_state_floats(const fe_resampler* rs);
/* the kernel the handle's last launch enqueued ("" before the first) */
const char* fe_resampler_last_kernel(const fe_resampler* rs);

/* B whole signals: row b is in_dev[b * in_stride + i], i < n_in, elements of in_format (FE_AUDIO_*); its fe_resampler_out_count outputs
 * go to out_dev[b * out_stride + m] as elements of out_format, and nothing else of a row is written.  n_in >= 1, B >= 1,
 * in_stride >= n_in, out_stride >= the output count.  Asynchronous on `stream`. */
int fe_resample(fe_resampler* rs, const void* in_dev, size_t in_stride, int in_format, long long n_in, void* out_dev, size_t out_stride,
                int out_format, int B, void* stream);

/* n packet streams in one launch.  Call stream i has a descriptor in DEVICE memory, read when the kernel runs: its state slot, the samples it
 * consumes now and the element offsets of its first input / output sample in the flat buffers in [in_count] / out [out_count].
 * State: state_dev [capacity][state_floats] floats, one row per slot -
 *     hist[K - 1]     the last K - 1 input samples as floats, oldest first
 *     2 words         the consumed sample count, low 32-bit word first
 *     padding         to a multiple of 4 floats
 * A zero row is a fresh stream; rows are plain data: copying a row moves a stream, zeroing it restarts one.
 * Per stream: n_in is clamped to [0, n_in_max]; the stream then emits p = M(consumed + n_in) - M(consumed) outputs.  A stream whose slot is
 * outside [0, capacity), or whose ranges [in_offset, in_offset + n_in) / [out_offset, out_offset + p) do not lie inside the buffers, is
 * SKIPPED: nothing of it is read, nothing written, its row untouched.  produced (may be NULL) is an int table [n] indexed by call stream,
 * device or page-locked host memory: p, and 0 for a skipped stream, written for every i.  Elements of out past a stream's p outputs are
 * not written.  One slot named twice in a call is undefined.  The call allocates nothing and synchronises nothing (after the handle's
 * first launch, above).
 * _pinned: in / out are page-locked HOST memory with a device mapping (the rules of fe_step_streams_pinned: pageable memory is refused
 * before any launch, the launch is asynchronous, synchronise the stream before reading out or rewriting in). */
typedef struct fe_resample_desc {    /* 24 bytes */
    int slot, n_in;
    long long in_offset, out_offset;
} fe_resample_desc;
int fe_resample_streams(fe_resampler* rs, const void* in, size_t in_count, int in_format, float* state_dev, int capacity,
                        const fe_resample_desc* desc_dev, void* out, size_t out_count, int out_format, int* produced, int n, int n_in_max,
                        void* stream);
int fe_resample_streams_pinned(fe_resampler* rs, const void* in, size_t in_count, int in_format, float* state_dev, int capacity,
                               const fe_resample_desc* desc_dev, void* out, size_t out_count, int out_format, int* produced, int n, int n_in_max,
                               void* stream);

/* The ring form of fe_resample_streams: the same call - state rows, n_in clamped to [0, n_in_max], p = M(consumed + n_in) - M(consumed)
 * outputs, produced, the _pinned twin, the same refusals in the same order - for streams whose samples live in RINGS inside the flat
 * buffers, such as the page-locked rings of a packet pool: sample i of a stream's input is element in_base + (in_pos + i) mod in_len of in,
 * output m of this call is element out_base + (out_pos + m) mod out_len of out; a packet and its outputs may wrap.  A flat buffer is the
 * special case pos = 0 with len at least the count.  The outputs are, bit for bit, those of fe_resample_streams on the same samples.
 * A stream is SKIPPED - nothing read, nothing written, its row untouched, produced[i] = 0 - unless its slot is in [0, capacity), its stored
 * count is one, in_len >= 1 and out_len >= 1, 0 <= in_pos < in_len and 0 <= out_pos < out_len, n_in <= in_len and p <= out_len, and the
 * whole of each ring, [base, base + len), lies inside [0, count) of its buffer.  No element outside a stream's ranges is written.
 * fe_resampler_last_kernel reports fe_resample_kernel<ring> or <ring,pinned>. */
typedef struct fe_resample_ring_desc {   /* 40 bytes */
    int slot, n_in;
    long long in_base, out_base;         /* element index of ring element 0 in in / out */
    int in_len, in_pos;                  /* ring length in elements; position of the first sample read, 0 <= in_pos < in_len */
    int out_len, out_pos;                /* ...; position of the first output written */
} fe_resample_ring_desc;
int fe_resample_rings(fe_resampler* rs, const void* in, size_t in_count, int in_format, float* state_dev, int capacity,
                      const fe_resample_ring_desc* desc_dev, void* out, size_t out_count, int out_format, int* produced, int n, int n_in_max,
                      void* stream);
int fe_resample_rings_pinned(fe_resampler* rs, const void* in, size_t in_count, int in_format, float* state_dev, int capacity,
                             const fe_resample_ring_desc* desc_dev, void* out, size_t out_count, int out_format, int* produced, int n, int n_in_max,
                             void* stream);

const char* fe_last_error(void);
const char* fe_version(void);
/* r6: the digest of the sources this library was built from (fastenhancer_amd/build.py::source_key: csrc/* and this header).  The Python binding refuses an
 * in-tree library whose key is not the tree's, and __graft_entry__.build() checks it after building: a stale object cache cannot pass for the shipped sources. */
const char* fe_build_key(void);

#ifdef __cplusplus
}
#endif
#endif /* FASTENHANCER_HIP_H */
