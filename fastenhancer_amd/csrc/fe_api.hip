// fe_api.hip — C ABI (include/fastenhancer_hip.h), handle management, weight packing and
// kernel dispatch for the FastEnhancer forward path on gfx950.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/fastenhancer_hip.h"
#include "fe_fragments.h"
#include "fe_impl.h"
#include "bsrnn_kernels.hip.h"
#include "fspen_kernels.hip.h"
#include "lisennet_kernels.hip.h"
#include "stft_kernels.hip.h"
#include "resample_kernels.hip.h"

// fe_last_step_kernel: the launchers (per-shape translation units included) name what they enqueue; a compute entry point
// clears the log when it starts and leaves it in its handle when it returns (KernelLogScope)
namespace fe {
namespace {
struct KernelLog { const char* name[16]; int n; };
thread_local KernelLog g_klog{};
}
void note_kernel(const char* name) {
    if (g_klog.n < 16) g_klog.name[g_klog.n] = name;
    if (g_klog.n < 17) ++g_klog.n;           // (17: more than the log holds)
}
}  // namespace fe

namespace {

thread_local std::string g_err;

// fe_set_option / fe_get_option.  `env`: the environment variable that sets the value NEW handles start with (A/B scripts under tools/);
// out-of-range or non-numeric values are ignored.
enum { OPT_BSRNN_ROLE_SPLIT = 0, OPT_BSRNN_SB_MIN, OPT_BSRNN_THREE_LAUNCH, OPT_BSRNN_OV_PROFILE, OPT_FSPEN_SB_MIN, OPT_LOW_LDS_COMPANION, OPT_BSRNN_FUSED, OPT_LISENNET_SB_MIN, OPT_COUNT };
struct OptionDef { const char* name; const char* env; int dflt, lo, hi; };
constexpr OptionDef kOptions[OPT_COUNT] = {
    {"bsrnn_role_split", "FE_BSRNN_OV", 1, 0, 1},
    {"bsrnn_stream_batch_min", "FE_BSRNN_SB", 2048, 0, 1 << 24},
    {"bsrnn_three_launch_step", "FE_BSRNN_SPLIT", 1, 0, 1},
    {"bsrnn_ov_profile", "FE_BSRNN_OV_PROF", 0, 0, 1},
    {"fspen_stream_batch_min", "FE_FSPEN_SB", 1536, 0, 1 << 24},
    {"low_lds_companion", "FE_LOWLDS", 1, 0, 1},
    {"bsrnn_fused_step", "FE_BSRNN_FUSED", 0, 0, 1},      // (measured negative: profiles/r6_bsrnn_fused_step.txt)
    {"lisennet_stream_batch_min", "FE_LISENNET_SB", 513, 0, 1 << 24},      // (2 x 256 + 1: from where the per-stream kernel needs a second round of workgroups - 219 us against the tiles' 193)
};
int env_int(const char* name, int dflt, int lo, int hi) {
    const char* e = std::getenv(name);
    if (!e || !*e) return dflt;
    char* end = nullptr;
    const long v = std::strtol(e, &end, 10);
    return (end && *end == 0 && v >= lo && v <= hi) ? (int)v : dflt;
}

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

// what an entry point returns after a launch that reported `e`
int launch_rc(hipError_t e) { return e == hipSuccess ? FE_OK : fail(FE_ERR_HIP, "kernel launch: %s", hipGetErrorString(e)); }

#define FE_HIP_CHECK(expr)                                                                  \
    do {                                                                                    \
        hipError_t _e = (expr);                                                             \
        if (_e != hipSuccess) return fail(FE_ERR_HIP, "%s: %s", #expr, hipGetErrorString(_e)); \
    } while (0)

struct Section {
    std::string name;
    size_t offset, count;
    std::vector<int> shape;
};

struct Dims {
    int C1, NL, C2, F2, KB, NFFT, HOP, F0, F1, HD;
    int ks[FE_MAX_KERNELS];
    int KT = 1;                // kernel_size_time (time_kernel variant)
    int FR = 0;                // 1: dprnn variant (sub-band GRU of C2 / 2 hidden units per direction instead of the attention)
    int LN = 0;                // 1: ln variant (GroupNorm after every conv, the reference's LayerNorm after the blocks' fc layers)
    int TA = 0;                // > 0: dptransformer variant (causal attention over the last TA frames instead of the time GRU)
    int BD = 0;                // 1: noncausal variant (bidirectional time GRU, rnn_fc over 2 C2; offline only, no caches)
    // model-state floats per stream: KB GRU states [F2][C2], or (dptransformer) 2 KB caches [F2][NH][TA][HD] + the ring head
    size_t hstate() const { return BD ? 0 : (size_t)KB * F2 * C2 * (TA ? 2 * TA : 1) + (TA ? 1 : 0); }
};

// ---------------------------------------------------------------------------- dispatch table
#define X(name, ...) extern "C" const fe::Impl* fe_impl_##name();
#ifdef FE_SHAPES_DEF         // a side build with a short shape list (build.py)
#include FE_SHAPES_DEF
#else
#include "fe_shapes.def"
#ifdef FE_LOCAL_DEF          // shapes added with `python -m fastenhancer_amd.build --add-shape ...`
#include FE_LOCAL_DEF
#endif
#endif
#undef X

#define XB(name, ...) extern "C" const fe::BImpl* fe_bimpl_##name();
#include "fe_bsrnn_shapes.def"
#undef XB
extern "C" const fe::FImpl* fe_fimpl_h256();
extern "C" const fe::LImpl* fe_limpl_h256();

const std::vector<const fe::BImpl*>& bimpls() {
    static const std::vector<const fe::BImpl*> v = {
#define XB(name, ...) fe_bimpl_##name(),
#include "fe_bsrnn_shapes.def"
#undef XB
    };
    return v;
}

const std::vector<const fe::Impl*>& impls() {
    static const std::vector<const fe::Impl*> v = {
#define X(name, ...) fe_impl_##name(),
#ifdef FE_SHAPES_DEF
#include FE_SHAPES_DEF
#else
#include "fe_shapes.def"
#ifdef FE_LOCAL_DEF
#include FE_LOCAL_DEF
#endif
#endif
#undef X
    };
    return v;
}

}  // namespace

struct fe_handle {
    fe_config cfg;
    Dims d;
    const fe::Impl* impl = nullptr;
    const fe::Impl* impl_many = nullptr;  // low-LDS companion (two workgroups per CU) for batches above #CUs streams, if compiled
    const fe::BImpl* bimpl = nullptr;     // arch == FE_ARCH_BSRNN
    const fe::FImpl* fimpl = nullptr;     // arch == FE_ARCH_FSPEN
    const fe::LImpl* limpl = nullptr;     // arch == FE_ARCH_LISENNET
    fe::BOffsets boff{};
    fe::SbOffsets sboff{};                    // stream-batched BSRNN layers (bsrnn_sb_kernels.hip.h), where built
    int packed_floats = 0;                    // floats of packed_dev (BSRNN)
    int device = 0;
    int max_wgs = 256;             // CUs of the device: one resident workgroup per CU (persistent grid above that)
    int pipe_frames = -1;          // fe_set_time_pipeline (-1: chosen from the model size)
    int offline_engine = FE_OFFLINE_AUTO;     // fe_set_offline_engine
    // fe_set_step_kernel / fe_set_option: which kernel a step dispatches.  The environment variables named in kOptions set the values NEW handles start
    // with (A/B runs of tools/ab_*.sh; a value outside the option's range, garbage included, is ignored) - nothing else in the library reads them.
    int step_kernel = FE_STEP_KERNEL_WG8;
    int opt[OPT_COUNT] = {};                  // kOptions order
    const char* last_kernels[16] = {};        // fe_last_step_kernel: what the last compute call enqueued (string literals of the launchers)
    int n_last_kernels = 0;
    const char* last_shape = nullptr;         // ... and the compiled shape record that launched it
    mutable std::string last_text;
    fe_handle() {
        for (int i = 0; i < OPT_COUNT; ++i) opt[i] = env_int(kOptions[i].env, kOptions[i].dflt, kOptions[i].lo, kOptions[i].hi);
        if (std::getenv("FE_NO_LOWLDS")) opt[OPT_LOW_LDS_COMPANION] = 0;      // (the older spelling tools/ab_lowlds.sh uses)
        step_kernel = env_int("FE_WG8", FE_STEP_KERNEL_WG8, FE_STEP_KERNEL_WAVES4, FE_STEP_KERNEL_WG8_PERSIST);
    }
    unsigned int* pipe_flags_dev = nullptr;   // fe_spec_step's frame counters [max_wgs][KB] (fe_offline keeps its own in the work buffer)
    unsigned long long* tb_probe_dev = nullptr;   // FE_TB_PROBE builds: phase clocks [4][kProbeSlots]
    hipStream_t host_streams[2] = {nullptr, nullptr};     // fe_step_host: copy-in / copy-out streams (lazy)
    hipEvent_t host_events[7] = {};                       // ... and its events
    int* ident_slots_dev = nullptr;           // fe_step_pinned: the identity slot list 0 .. ident_slots - 1 (grow-only)
    int ident_slots = 0;
    float* tb_work_dev = nullptr;             // fe_spec_step on the time-batched engine: grow-only work buffer
    float* spec_ring_dev = nullptr;           // fe_spec_step, dptransformer, time-pipelined: the K / V rings of TA + P slots per pair (grow-only)
    size_t spec_ring_floats = 0;
    unsigned int* bsync_dev = nullptr;        // BSRNN fused per-hop step: barrier counters of the sixteen-stream tiles [kSyncTiles][2] (zeroed once; monotonic)
    float* sb_dev = nullptr;                  // stream-batched per-hop step of BSRNN / FSPEN / LiSenNet: its scratch (ensure_sb_scratch)
    int sb_streams = 0;                       // (grow-only, sized by fe_state_init / the first step of a larger batch)
    size_t tb_work_floats = 0;
    std::vector<Section> sections;
    size_t blob_floats = 0;
    float* packed_dev = nullptr;   // the weight banks: n_banks packed buffers, bank k at packed_dev + k * bank_stride (allocated by the first load)
    int n_banks = 1;               // fe_set_weight_banks
    size_t bank_stride = 0;        // floats from one bank to the next: the packed size rounded up to 64 floats (set with packed_dev)
    std::vector<char> bank_loaded = std::vector<char>(1, 0);      // [n_banks]; bank 0's is `loaded`
    float* tables_dev = nullptr;  // [window | window_istft | twiddle] for the stand-alone STFT launches (lazy)
    float* skip_dev = nullptr;     // scratch for shapes whose skips do not fit in LDS
    int skip_streams = 0;
    bool loaded = false;
    std::vector<float> window, window_istft, twiddle;
};

namespace {

void add_section(fe_handle* h, const std::string& name, std::vector<int> shape) {
    size_t n = 1;
    for (int s : shape) n *= (size_t)s;
    size_t off = (h->blob_floats + 3) & ~(size_t)3;
    h->sections.push_back(Section{name, off, n, shape});
    h->blob_floats = off + n;
}

// the ln variant's fused state_dict (models/fastenhancer/ln/model.py:416-518 after remove_weight_reparameterizations; the final
// conv as dec_post.2 with its scale folded in, like the default model's): convs with their own biases, every norm layer kept
void build_sections_ln(fe_handle* h) {
    const Dims& d = h->d;
    char nm[128];
    auto wb = [&](const std::string& p, std::vector<int> wshape, bool bias = true) {
        add_section(h, p + ".weight", wshape);
        if (bias) add_section(h, p + ".bias", {wshape[0]});
    };
    wb("enc_pre.0", {d.C1, 8, 2}); wb("enc_pre.1", {d.C1});
    for (int i = 0; i < d.NL; ++i) {
        snprintf(nm, sizeof nm, "encoder.%d.0", i); wb(nm, {d.C1, d.C1, 3});
        snprintf(nm, sizeof nm, "encoder.%d.1", i); wb(nm, {d.C1});
    }
    add_section(h, "rf_pre.0.weight", {d.F2, d.F1});
    wb("rf_pre.1", {d.C2, d.C1, 1}); wb("rf_pre.2", {d.C2});
    for (int k = 0; k < d.KB; ++k) {
        auto key = [&](const char* s) { snprintf(nm, sizeof nm, "rf_block.%d.%s", k, s); return std::string(nm); };
        if (k == 0) add_section(h, key("pe"), {d.F2, d.C2});
        add_section(h, key("rnn.weight_ih_l0"), {3 * d.C2, d.C2});
        add_section(h, key("rnn.weight_hh_l0"), {3 * d.C2, d.C2});
        add_section(h, key("rnn.bias_ih_l0"), {3 * d.C2});
        add_section(h, key("rnn.bias_hh_l0"), {3 * d.C2});
        add_section(h, key("rnn_fc.weight"), {d.C2, d.C2});
        wb(key("rnn_post_norm"), {d.C2});
        add_section(h, key("attn.qkv.weight"), {3 * d.C2, d.C2});
        add_section(h, key("attn_fc.weight"), {d.C2, d.C2});
        wb(key("attn_post_norm"), {d.C2});
    }
    add_section(h, "rf_post.0.weight", {d.F1, d.F2});
    wb("rf_post.1", {d.C1, d.C2, 1}); wb("rf_post.2", {d.C1});
    for (int i = 0; i < d.NL; ++i) {
        snprintf(nm, sizeof nm, "decoder.%d.0", i); wb(nm, {d.C1, 2 * d.C1, 1});
        snprintf(nm, sizeof nm, "decoder.%d.1", i); wb(nm, {d.C1});
        snprintf(nm, sizeof nm, "decoder.%d.3", i); wb(nm, {d.C1, d.C1, 3}, false);
        snprintf(nm, sizeof nm, "decoder.%d.4", i); wb(nm, {d.C1});
    }
    wb("dec_post.0", {d.C1, 2 * d.C1, 1}, false); wb("dec_post.1", {d.C1});
    add_section(h, "dec_post.2.weight", {d.C1, 2, 8});
    add_section(h, "dec_post.2.bias", {2});
}

void build_sections(fe_handle* h) {
    const Dims& d = h->d;
    if (d.LN) { build_sections_ln(h); return; }
    char nm[128];
    add_section(h, "enc_pre.0.weight", {d.C1, 8, 2});
    add_section(h, "enc_pre.0.bias", {d.C1});
    for (int i = 0; i < d.NL; ++i) {
        snprintf(nm, sizeof nm, "encoder.%d.0.weight", i);
        if (d.KT > 1) add_section(h, nm, {d.C1, d.C1, d.KT, 3}); else add_section(h, nm, {d.C1, d.C1, 3});
        snprintf(nm, sizeof nm, "encoder.%d.0.bias", i); add_section(h, nm, {d.C1});
    }
    add_section(h, "rf_pre.0.weight", {d.F2, d.F1});
    add_section(h, "rf_pre.1.weight", {d.C2, d.C1, 1});
    add_section(h, "rf_pre.1.bias", {d.C2});
    if (d.TA) add_section(h, "time_pe", {4, d.TA + 1});      // the dptransformer model's positional bias (its `pe` parameter)
    for (int k = 0; k < d.KB; ++k) {
        auto key = [&](const char* s) { snprintf(nm, sizeof nm, "rf_block.%d.%s", k, s); return std::string(nm); };
        if (k == 0 && !d.FR) add_section(h, key("pe"), {d.F2, d.C2});
        if (d.TA) add_section(h, key("time_attn.qkv.weight"), {3 * d.C2, d.C2});
        else {
        for (const char* sfx : {"", "_reverse"}) {
            if (sfx[0] && !d.BD) break;
            add_section(h, key((std::string("rnn.weight_ih_l0") + sfx).c_str()), {3 * d.C2, d.C2});
            add_section(h, key((std::string("rnn.weight_hh_l0") + sfx).c_str()), {3 * d.C2, d.C2});
            add_section(h, key((std::string("rnn.bias_ih_l0") + sfx).c_str()), {3 * d.C2});
            add_section(h, key((std::string("rnn.bias_hh_l0") + sfx).c_str()), {3 * d.C2});
        }
        }
        add_section(h, key("rnn_fc.weight"), {d.C2, d.BD ? 2 * d.C2 : d.C2});
        add_section(h, key("rnn_fc.bias"), {d.C2});
        if (d.FR) {     // DPRNN's fused state_dict (models/fastenhancer/dprnn/model.py:159-161), module names as the default model's
            const int H = d.C2 / 2;
            for (const char* sfx : {"", "_reverse"}) {
                add_section(h, key((std::string("frnn.weight_ih_l0") + sfx).c_str()), {3 * H, d.C2});
                add_section(h, key((std::string("frnn.weight_hh_l0") + sfx).c_str()), {3 * H, H});
                add_section(h, key((std::string("frnn.bias_ih_l0") + sfx).c_str()), {3 * H});
                add_section(h, key((std::string("frnn.bias_hh_l0") + sfx).c_str()), {3 * H});
            }
            add_section(h, key("frnn_fc.weight"), {d.C2, d.C2});
            add_section(h, key("frnn_fc.bias"), {d.C2});
            continue;
        }
        add_section(h, key("attn.qkv.weight"), {3 * d.C2, d.C2});
        add_section(h, key("attn_fc.weight"), {d.C2, d.C2});
        add_section(h, key("attn_fc.bias"), {d.C2});
    }
    add_section(h, "rf_post.0.weight", {d.F1, d.F2});
    add_section(h, "rf_post.1.weight", {d.C1, d.C2, 1});
    add_section(h, "rf_post.1.bias", {d.C1});
    for (int i = 0; i < d.NL; ++i) {
        snprintf(nm, sizeof nm, "decoder.%d.0.weight", i); add_section(h, nm, {d.C1, 2 * d.C1, 1});
        snprintf(nm, sizeof nm, "decoder.%d.0.bias", i); add_section(h, nm, {d.C1});
        snprintf(nm, sizeof nm, "decoder.%d.2.weight", i);
        if (d.KT > 1) add_section(h, nm, {d.C1, d.C1, d.KT, 3}); else add_section(h, nm, {d.C1, d.C1, 3});
        snprintf(nm, sizeof nm, "decoder.%d.2.bias", i); add_section(h, nm, {d.C1});
    }
    add_section(h, "dec_post.0.weight", {d.C1, 2 * d.C1, 1});
    add_section(h, "dec_post.0.bias", {d.C1});
    add_section(h, "dec_post.2.weight", {d.C1, 2, 8});
    add_section(h, "dec_post.2.bias", {2});
}

// Window tables, ONNXSTFT.__init__ (functional/audio_modules.py:207-235).
void build_tables(fe_handle* h) {
    const int N = h->cfg.n_fft, H = h->cfg.hop_size, W = h->cfg.win_size;
    std::vector<float> win(N, 0.0f);
    const int pad = N - W;
    for (int i = 0; i < W; ++i) {   // torch.hann_window(W), periodic
        double v = 0.5 - 0.5 * std::cos(2.0 * M_PI * (double)i / (double)W);
        win[pad / 2 + i] = (float)v;
    }
    const int K = (N + H - 1) / H;
    const int L = H * (2 * K - 1) + (N - H);
    std::vector<float> acc(L, 0.0f);
    for (int j = 0; j < 2 * K - 1; ++j)
        for (int n = 0; n < N; ++n) acc[j * H + n] += win[n] * win[n];
    std::vector<float> wi(N);
    for (int n = 0; n < N; ++n) wi[n] = win[n] / acc[(K - 1) * H + n];
    h->window = win;
    h->window_istft = wi;
    h->twiddle.resize(N);   // N/2 complex
    for (int k = 0; k < N / 2; ++k) {
        double ang = -2.0 * M_PI * (double)k / (double)N;
        h->twiddle[2 * k] = (float)std::cos(ang);
        h->twiddle[2 * k + 1] = (float)std::sin(ang);
    }
}

// what every fe_create path shares: the handle, its device and CU count, its window tables (the caller adds its kernels and sections)
fe_handle* new_handle(const fe_config* cfg, const Dims& d) {
    fe_handle* h = new fe_handle();
    h->cfg = *cfg;
    h->d = d;
    if (hipGetDevice(&h->device) != hipSuccess) h->device = -1;   // no GPU: sections/tables still usable
    else {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device) == hipSuccess && cus > 0) h->max_wgs = cus;
    }
    build_tables(h);
    return h;
}

// constant operands of the matrix-core DFT (fe::Dft in fe_kernels.hip.h), N = N1 * 32, at the four given offsets of p
void pack_dft_constants(fe::frag::Buffer& p, int N, int dft1, int dft2, int dft3, int dft4) {
    {
        const int N1 = N / 32, KC = N1 / 2, MT = N1 / 16;
        auto c32 = [](int a, int b) { return std::cos(2.0 * M_PI * (double)((a * b) % 32) / 32.0); };
        auto s32 = [](int a, int b) { return std::sin(2.0 * M_PI * (double)((a * b) % 32) / 32.0); };
        auto c1 = [&](int a, int b) { return std::cos(2.0 * M_PI * (double)((a * b) % N1) / (double)N1); };
        auto s1 = [&](int a, int b) { return std::sin(2.0 * M_PI * (double)((a * b) % N1) / (double)N1); };
        for (int q = 0; q < 2; ++q) {
            // forward, 32-point stage: B[k = n2][n = k2] = Re (q = 0) / Im (q = 1) of W_32^(n2 k2)
            p.pack_b(dft1 + q * (2 * 8 * 64), 32, 32, [&](int k, int n) { return (float)(q == 0 ? c32(k, n) : -s32(k, n)); });
            // forward, N1-point stage, output half q: A[m = k1][k-step a*4MT + 4i + r, lane group lg]  <->  half a of
            // G', row n1 = 16 i + 4 lg + r:   Re X: [cos | sin],  Im X: [-sin | cos]
            p.pack_a(dft2 + q * (KC * 64), 16, 2 * N1, [&](int m, int k) {
                const int ks = k / 4, lg = k % 4, a = ks / (4 * MT), i = (ks % (4 * MT)) / 4, r = ks % 4;
                const int n1 = 16 * i + 4 * lg + r;
                if (q == 0) return (float)(a ? s1(m, n1) : c1(m, n1));
                return (float)(a ? c1(m, n1) : -s1(m, n1));
            });
            // inverse, N1-point stage (transposed), half q of H: B[k = (b, k1)][n = n1]:  Re H: [cos | -sin],  Im H: [sin | cos]
            p.pack_b(dft3 + q * (MT * KC * 64), 2 * N1, N1, [&](int k, int n) {
                const int b = k / N1, k1 = k % N1;
                if (q == 0) return (float)(b ? -s1(n, k1) : c1(n, k1));
                return (float)(b ? c1(n, k1) : s1(n, k1));
            });
            // inverse, 32-point stage (with the 1/N of irfft), per wave (p = q, jt): B[k-step a*4 + r, lane group lg][n = li]
            // <-> half a of H', k2 = 16 jt + 4 lg + r, output sample column n2 = 16 p + li:  cos / N (a = 0), -sin / N (a = 1)
            for (int jt = 0; jt < 2; ++jt)
                p.pack_b(dft4 + (q * 2 + jt) * (8 * 64), 32, 16, [&](int k, int n) {
                    const int ks = k / 4, lg = k % 4, a = ks / 4, r = ks % 4;
                    const int k2 = 16 * jt + 4 * lg + r, n2 = 16 * q + n;
                    return (float)((a ? -s32(k2, n2) : c32(k2, n2)) / (double)N);
                });
        }
    }
}

// the fused blob by section name: S("enc_pre.0.weight")
struct Blob {
    const fe_handle* h;
    const float* v;
    const float* operator()(const std::string& name) const {
        for (const Section& s : h->sections)
            if (s.name == name) return v + s.offset;
        return nullptr;
    }
};

// [window | window_istft | twiddle] of the handle, where a family's offset table wants them
void pack_stft_tables(fe::frag::Buffer& p, const fe_handle* h, int window, int window_istft, int twiddle) {
    p.raw(window, h->window.size(), h->window.data());
    p.raw(window_istft, h->window_istft.size(), h->window_istft.data());
    p.raw(twiddle, h->twiddle.size(), h->twiddle.data());
}

// FastEnhancer: fragments (fe_fragments.h) at the compile-time offsets of fe::Pack<S>::v (the kernel uses the same table)
int pack_weights(fe_handle* h, const Blob& S, std::vector<float>* out) {
    const Dims& d = h->d;
    const int C1 = d.C1, C2 = d.C2, F1 = d.F1, F2 = d.F2;
    const fe::PackedOffsets& o = *h->impl->off;
    fe::frag::Buffer p((size_t)o.total);
    char nm[128];
    // (Co, Ci, 3), or (Co, Ci, KT, 3) for the time_kernel variant: one B operand per time tap, k = freq_tap*Ci + ci.
    // Units are in consumption order: unit 0 multiplies the CURRENT frame = time index KT-1 of the causal kernel, unit j the
    // frame j steps back = time index KT-1-j
    const int KT = d.KT;
    auto pack_k3 = [&](const int* offs, const float* w) {
        for (int j = 0; j < KT; ++j) {
            const int dt = KT - 1 - j;
            p.pack_b(offs[j], 3 * C1, C1, [&](int k, int n) { return w[((size_t)(n * C1 + (k % C1)) * KT + dt) * 3 + (k / C1)]; });
        }
    };
    auto pack_1x1 = [&](int off, const float* w, int Ci, int Co) {   // (Co, Ci[,1]): B[k=ci][n=co]
        p.pack_b(off, Ci, Co, [&](int k, int n) { return w[n * Ci + k]; });
    };
    {   // enc_pre: weight (C1, 8, 2): B[k = t*8 + ch][n = co] = W[co][ch][t]
        const float* w = S("enc_pre.0.weight");
        p.pack_b(o.enc_pre_w, 16, C1, [&](int k, int n) { return w[(n * 8 + (k & 7)) * 2 + (k >> 3)]; });
        p.rep4(o.enc_pre_b, C1, S("enc_pre.0.bias"));
    }
    for (int i = 0; i < d.NL; ++i) {
        snprintf(nm, sizeof nm, "encoder.%d.0.weight", i); pack_k3(&o.enc_w[i * KT], S(nm));
        snprintf(nm, sizeof nm, "encoder.%d.0.bias", i); p.rep4(o.enc_b[i], C1, S(nm));
    }
    {   // rf_pre: Linear (F2, F1) as A operand, then 1x1 conv (C2, C1)
        const float* w = S("rf_pre.0.weight");
        p.pack_a(o.rfpre_lin, F2, F1, [&](int m, int k) { return w[m * F1 + k]; });
        pack_1x1(o.rfpre_w, S("rf_pre.1.weight"), C1, C2);
        p.rep4(o.rfpre_b, C2, S("rf_pre.1.bias"));
    }
    if (d.TA) {     // [NH][L + 1] -> [NH][32]
        const float* tp = S("time_pe");
        for (int hh = 0; hh < 4; ++hh)
            for (int j = 0; j <= d.TA; ++j) p[o.tpe + hh * 32 + j] = tp[hh * (d.TA + 1) + j];
    }
    for (int k = 0; k < d.KB; ++k) {
        auto key = [&](const char* s) { snprintf(nm, sizeof nm, "rf_block.%d.%s", k, s); return std::string(nm); };
        if (d.TA) pack_1x1(o.blk_tqkv[k], S(key("time_attn.qkv.weight")), C2, 3 * C2);
        else if (!d.BD)
        {   // GRU (3*C2, C2), gate order r,z,n: one padded column block per gate
            const int gsz = fe::ceil_div(C2, 16) * (C2 / 4) * 64, bsz = fe::round_up(C2, 16);
            const float* wih = S(key("rnn.weight_ih_l0"));
            const float* whh = S(key("rnn.weight_hh_l0"));
            const float* bih = S(key("rnn.bias_ih_l0"));
            const float* bhh = S(key("rnn.bias_hh_l0"));
            if (o.gru_flat) {   // one (3 C2)-column matrix, rows r | z | n as stored by nn.GRU
                pack_1x1(o.blk_wih[k], wih, C2, 3 * C2);
                pack_1x1(o.blk_whh[k], whh, C2, 3 * C2);
                p.raw(o.blk_bih[k], 3 * C2, bih);
                p.raw(o.blk_bhh[k], 3 * C2, bhh);
            } else
            for (int g = 0; g < 3; ++g) {
                pack_1x1(o.blk_wih[k] + g * gsz, wih + (size_t)g * C2 * C2, C2, C2);
                pack_1x1(o.blk_whh[k] + g * gsz, whh + (size_t)g * C2 * C2, C2, C2);
                p.raw(o.blk_bih[k] + g * bsz, C2, bih + g * C2);
                p.raw(o.blk_bhh[k] + g * bsz, C2, bhh + g * C2);
            }
        }
        if (o.u8_gx[k] != 0) {
            // 512-thread per-hop kernel (fe_frame8.hip.h, Shape::G8P): the block weights as LDS-staged units (PackedOffsets::u8_*):
            // plain B fragments followed by the tiles' start values [tile][16].
            const float* wih = S(key("rnn.weight_ih_l0"));
            const float* whh = S(key("rnn.weight_hh_l0"));
            const float* bih = S(key("rnn.bias_ih_l0"));
            const float* bhh = S(key("rnn.bias_hh_l0"));
            const int NG = C2 / 16, R = C2 % 16, NT = 3 * NG + 1, KS = C2 / 4;
            // tile t, column c -> row of the (rows, C2) weight matrix (-1: padding); bias(t, c)
            // (rscale(row): the gate rows carry -log2 e (r, z) / 2 log2 e (n) so that sigma / tanh are one exp2 + rcp of the accumulator)
            auto pack_u8 = [&](int off, int ntiles, const float* w, auto&& wrow, auto&& bias, auto&& rscale) {
                p.tiles(off, ntiles, KS, [&](int t, int c, int kk) { const int row = wrow(t, c); return row >= 0 ? w[(size_t)row * C2 + kk] * rscale(row) : 0.0f; });
                p.rows((size_t)off + (size_t)ntiles * KS * 64, ntiles, [&](int t, int c) { const int row = wrow(t, c); return row >= 0 ? bias(t, c) * rscale(row) : 0.0f; });
            };
            auto one = [](int) { return 1.0f; };
            auto gscale = [&](int row) { return row < 2 * C2 ? fe::kGateRZ : fe::kGateN; };
            // channel-grouped gate tiles: tile 3 G + gate: column c <-> channel 16 G + c of that gate; the last tile: columns [0, R) r,
            // [R, 2 R) z, [2 R, 3 R) n of the R = C2 % 16 left-over channels
            auto grow = [&](int t, int c) -> int {
                if (t < 3 * NG) return (t % 3) * C2 + 16 * (t / 3) + c;
                return c < 3 * R ? (c / R) * C2 + 16 * NG + c % R : -1;
            };
            auto shared = [&](int t) { return t < 3 * NG && t % 3 < 2; };      // pure r / z tile: x and h halves in one accumulator
            pack_u8(o.u8_gx[k], NT, wih, grow, [&](int t, int c) { const int r = grow(t, c); return bih[r] + (shared(t) ? bhh[r] : 0.0f); }, gscale);
            pack_u8(o.u8_gh[k], NT, whh, grow, [&](int t, int c) { const int r = grow(t, c); return shared(t) ? 0.0f : bhh[r]; }, gscale);
            auto plain = [&](int ncols) { return [ncols](int t, int c) { return 16 * t + c < ncols ? 16 * t + c : -1; }; };
            const float* f1b = S(key("rnn_fc.bias"));
            const float* f2b = S(key("attn_fc.bias"));
            pack_u8(o.u8_f1[k], fe::ceil_div(C2, 16), S(key("rnn_fc.weight")), plain(C2), [&](int t, int c) { return f1b[16 * t + c]; }, one);
            pack_1x1(o.u8_q[k], S(key("attn.qkv.weight")), C2, 3 * C2);      // qkv: fragments only (the unit has no start values)
            pack_u8(o.u8_f2[k], fe::ceil_div(C2, 16), S(key("attn_fc.weight")), plain(C2), [&](int t, int c) { return f2b[16 * t + c]; }, one);
        }
        if (h->impl->tb && !d.TA) {
            // time-batched engine (tb_kernels.hip.h): per direction the input weights as ONE flat (3 C2)-column matrix (rows r | z | n as
            // stored by nn.GRU) with the bias b_ih + (r, z) b_hh, the hidden weights per gate, b_hn
            const int gsz = fe::ceil_div(C2, 16) * (C2 / 4) * 64;
            for (int dir = 0; dir < (d.BD ? 2 : 1); ++dir) {
                const char* sfx = dir ? "_reverse" : "";
                const float* wih = S(key((std::string("rnn.weight_ih_l0") + sfx).c_str()));
                const float* whh = S(key((std::string("rnn.weight_hh_l0") + sfx).c_str()));
                const float* bih = S(key((std::string("rnn.bias_ih_l0") + sfx).c_str()));
                const float* bhh = S(key((std::string("rnn.bias_hh_l0") + sfx).c_str()));
                pack_1x1(o.tb_wih[k][dir], wih, C2, 3 * C2);
                for (int c = 0; c < 3 * C2; ++c) p[(size_t)o.tb_bx[k][dir] + c] = bih[c] + (c < 2 * C2 ? bhh[c] : 0.0f);
                for (int g = 0; g < 3; ++g) pack_1x1(o.tb_whh[k][dir] + g * gsz, whh + (size_t)g * C2 * C2, C2, C2);
                p.raw(o.tb_bhn[k][dir], C2, bhh + 2 * C2);
            }
            if (d.BD) pack_1x1(o.tb_fc1_w[k], S(key("rnn_fc.weight")), 2 * C2, C2);
        }
        if (!d.BD) pack_1x1(o.blk_fc1_w[k], S(key("rnn_fc.weight")), C2, C2);
        if (!d.LN) p.raw(o.blk_fc1_b[k], C2, S(key("rnn_fc.bias")));      // (ln variant: the fc layers have no bias, their LayerNorm's is in the ln tables)
        if (d.FR) {
            // sub-band GRU: the input weights of both directions as one (3 C2)-column matrix [direction][r|z|n][unit] in the qkv
            // slot, its bias = b_ih + (r, z only) b_hh; hidden weights [direction][j][gate][unit]; b_hn.  (The block has no
            // positional embedding: blk_pe stays zero.)
            const int H = C2 / 2;
            std::vector<float> wih((size_t)3 * C2 * C2), bi((size_t)3 * C2);
            for (int dir = 0; dir < 2; ++dir) {
                const char* sfx = dir ? "_reverse" : "";
                const float* w = S(key((std::string("frnn.weight_ih_l0") + sfx).c_str()));
                const float* whh = S(key((std::string("frnn.weight_hh_l0") + sfx).c_str()));
                const float* bih = S(key((std::string("frnn.bias_ih_l0") + sfx).c_str()));
                const float* bhh = S(key((std::string("frnn.bias_hh_l0") + sfx).c_str()));
                std::copy(w, w + (size_t)3 * H * C2, wih.begin() + (size_t)dir * 3 * H * C2);
                for (int r = 0; r < 3 * H; ++r) bi[(size_t)dir * 3 * H + r] = bih[r] + (r < 2 * H ? bhh[r] : 0.0f);
                const size_t dst = o.blk_fhh[k] + (size_t)dir * H * 3 * H;
                for (int j = 0; j < H; ++j)
                    for (int g = 0; g < 3; ++g)
                        for (int u = 0; u < H; ++u) p[dst + ((size_t)j * 3 + g) * H + u] = whh[((size_t)g * H + u) * H + j];
                for (int u = 0; u < H; ++u) p[o.blk_fbhn[k] + (size_t)dir * H + u] = bhh[2 * H + u];
            }
            pack_1x1(o.blk_qkv[k], wih.data(), C2, 3 * C2);
            p.raw(o.blk_qkv_b[k], 3 * C2, bi.data());
            pack_1x1(o.blk_fc2_w[k], S(key("frnn_fc.weight")), C2, C2);
            p.raw(o.blk_fc2_b[k], C2, S(key("frnn_fc.bias")));
            continue;
        }
        if (k == 0) p.raw(o.blk_pe, (size_t)F2 * C2, S(key("pe")));
        pack_1x1(o.blk_qkv[k], S(key("attn.qkv.weight")), C2, 3 * C2);
        pack_1x1(o.blk_fc2_w[k], S(key("attn_fc.weight")), C2, C2);
        if (!d.LN) p.raw(o.blk_fc2_b[k], C2, S(key("attn_fc.bias")));
    }
    {
        const float* w = S("rf_post.0.weight");   // (F1, F2)
        p.pack_a(o.rfpost_lin, F1, F2, [&](int m, int k) { return w[m * F2 + k]; });
        p.raw(o.rfpost_w, (size_t)C1 * C2, S("rf_post.1.weight"));      // plain copies: the debug dump of the rf_post stage
        p.raw(o.rfpost_b, C1, S("rf_post.1.bias"));
        if (d.LN) {     // its own staged unit: a GroupNorm sits between it and decoder layer 0
            pack_1x1(o.rfpost1_w, S("rf_post.1.weight"), C2, C1);
            p.rep4(o.rfpost1_b, C1, S("rf_post.1.bias"));
        }
    }
    const std::vector<float> zeros_c1((size_t)C1, 0.0f);
    for (int i = 0; i < d.NL; ++i) {
        if (i == 0 && !d.LN) {
            // rf_post's 1x1 conv (C2 -> C1, affine, no activation) feeds only this layer's x half: folded in.
            //   v = Wd_x (Wrp y + brp) + Wd_s skip + bd  =  (Wd_x Wrp) y + Wd_s skip + (bd + Wd_x brp)
            // K = C2 (filterbank output, true scale: weights carry kSiluScale) + C1 (skip, already scaled)
            const float* wrp = S("rf_post.1.weight");     // (C1, C2)
            const float* brp = S("rf_post.1.bias");
            const float* wd = S("decoder.0.0.weight");    // (C1, 2 C1): [n][0 .. C1) x, [n][C1 .. 2 C1) skip
            const float* bd = S("decoder.0.0.bias");
            std::vector<float> wf((size_t)C1 * C2), bf(C1);
            for (int n = 0; n < C1; ++n) {
                for (int k = 0; k < C2; ++k) {
                    double acc = 0.0;
                    for (int m = 0; m < C1; ++m) acc += (double)wd[(size_t)n * 2 * C1 + m] * wrp[(size_t)m * C2 + k];
                    wf[(size_t)n * C2 + k] = (float)(acc * fe::kSiluScale);
                }
                double acc = bd[n];
                for (int m = 0; m < C1; ++m) acc += (double)wd[(size_t)n * 2 * C1 + m] * brp[m];
                bf[n] = (float)acc;
            }
            p.pack_b(o.dec1_w[0], C2 + C1, C1, [&](int k, int n) { return k < C2 ? wf[(size_t)n * C2 + k] : wd[(size_t)n * 2 * C1 + C1 + (k - C2)]; });
            p.rep4(o.dec1_b[0], C1, bf.data());
        } else {
        snprintf(nm, sizeof nm, "decoder.%d.0.weight", i); pack_1x1(o.dec1_w[i], S(nm), 2 * C1, C1);
        snprintf(nm, sizeof nm, "decoder.%d.0.bias", i); p.rep4(o.dec1_b[i], C1, S(nm));
        }
        if (d.LN) {     // (the k = 3 conv is module 3 there and has no bias)
            snprintf(nm, sizeof nm, "decoder.%d.3.weight", i); pack_k3(&o.dec3_w[i * KT], S(nm));
            p.rep4(o.dec3_b[i], C1, zeros_c1.data());
            continue;
        }
        snprintf(nm, sizeof nm, "decoder.%d.2.weight", i); pack_k3(&o.dec3_w[i * KT], S(nm));
        snprintf(nm, sizeof nm, "decoder.%d.2.bias", i); p.rep4(o.dec3_b[i], C1, S(nm));
    }
    pack_1x1(o.post1_w, S("dec_post.0.weight"), 2 * C1, C1);
    p.rep4(o.post1_b, C1, d.LN ? zeros_c1.data() : S("dec_post.0.bias"));
    if (d.LN) {     // gain / bias of the norm sites, Shape::LN_SITES order
        int q = 0;
        auto site = [&](const std::string& prefix, int C) {
            p.raw(o.ln_g[q], C, S(prefix + ".weight"));
            p.raw(o.ln_b[q], C, S(prefix + ".bias"));
            ++q;
        };
        site("enc_pre.1", C1);
        for (int i = 0; i < d.NL; ++i) { snprintf(nm, sizeof nm, "encoder.%d.1", i); site(nm, C1); }
        site("rf_pre.2", C2);
        for (int k = 0; k < d.KB; ++k) {
            snprintf(nm, sizeof nm, "rf_block.%d.rnn_post_norm", k); site(nm, C2);
            snprintf(nm, sizeof nm, "rf_block.%d.attn_post_norm", k); site(nm, C2);
        }
        site("rf_post.2", C1);
        for (int i = 0; i < d.NL; ++i) {
            snprintf(nm, sizeof nm, "decoder.%d.1", i); site(nm, C1);
            snprintf(nm, sizeof nm, "decoder.%d.4", i); site(nm, C1);
        }
        site("dec_post.1", C1);
    }
    {   // transposed conv weight (C1, 2, 8): B[k = ci][n = co*8 + j]
        const float* w = S("dec_post.2.weight");
        p.pack_b(o.post_t_w, C1, 16, [&](int k, int n) { return w[k * 16 + n]; });
        p.raw(o.post_t_b, 2, S("dec_post.2.bias"));
    }
    {   // scaled conv trunk (fe_kernels.hip.h, kSiluScale): biases of the SiLU layers, entry weights, exit weights
        const float c = d.LN ? 1.0f : fe::kSiluScale;      // (ln variant: no scaling - a norm layer follows every conv)
        auto szB = [](int K, int N) { return (size_t)fe::ceil_div(N, 16) * (K / 4) * 64; };
        auto scale = [&](int off, size_t n, float f) { for (size_t i = 0; i < n; ++i) p[(size_t)off + i] *= f; };
        scale(o.enc_pre_w, szB(16, C1), c); scale(o.enc_pre_b, 4 * C1, c);       // (biases: 4x replicated tables)
        for (int i = 0; i < d.NL; ++i) { scale(o.enc_b[i], 4 * C1, c); scale(o.dec1_b[i], 4 * C1, c); scale(o.dec3_b[i], 4 * C1, c); }
        scale(o.rfpre_w, szB(C1, C2), 1.0f / c);                                  // encoder -> RNNFormer: back to true scale
        // (RNNFormer -> decoder: rf_post's 1x1 is folded into decoder.0.0 above, with the scale)
        scale(o.post1_b, 4 * C1, c);
        scale(o.post_t_w, szB(C1, 16), 1.0f / c);                                 // transposed conv: true-scale mask
    }
    if (o.act_p > 0) p[(size_t)o.act_p] = h->cfg.activation_param;            // LeakyReLU negative_slope / ELU alpha (Shape::EPP)
    pack_stft_tables(p, h, o.window, o.window_istft, o.twiddle);
    pack_dft_constants(p, h->cfg.n_fft, o.dft1, o.dft2, o.dft3, o.dft4);
    // a copy of [beg, end) delta floats on, in which tiles are then regrouped to k4 order (fe_fragments.h) for 16-byte fetches
    auto copy_region = [&](int beg, int end, int delta) { for (int i = beg; i < end; ++i) p[(size_t)i + delta] = p[i]; };
    if (o.k4_delta != 0) {
        // Register-resident block weights (fe::Shape::REGW): a second copy of the block-weight region with its B-operand tiles in k4 order
        // (the KS % 4 remainder plain) - fe::TokW
        copy_region(o.blk_wih[0], o.blk_end, o.k4_delta);
        const int KS = C2 / 4, NTC = fe::ceil_div(C2, 16), NT3 = fe::ceil_div(3 * C2, 16);
        auto regroup = [&](int off, int tiles) { p.regroup_k4((size_t)off + o.k4_delta, off, tiles, KS, 0, KS); };
        for (int k = 0; k < d.KB; ++k) {
            regroup(o.blk_wih[k], 3 * NTC); regroup(o.blk_whh[k], 3 * NTC);
            regroup(o.blk_fc1_w[k], NTC); regroup(o.blk_qkv[k], NT3); regroup(o.blk_fc2_w[k], NTC);
            if (d.TA) regroup(o.blk_tqkv[k], NT3);
        }
    }
    if (o.conv_k4_delta != 0) {
        // Time-batched engine (r4w): a copy of the conv units whose weight tiles are in k4 order (tb_kernels.hip.h::conv_gemm; the biases
        // and the filterbanks in the copy stay as they are).  Must run AFTER every conv weight is packed.
        copy_region(o.u_off[0], o.u_off[o.n_units - 1] + o.u_size[o.n_units - 1], o.conv_k4_delta);
        auto regroup_c = [&](int off, int tiles, int KS) { p.regroup_k4((size_t)off + o.conv_k4_delta, off, tiles, KS, 0, KS); };
        const int NTC = fe::ceil_div(C1, 16), KSC = C1 / 4, KS2 = C2 / 4;
        regroup_c(o.enc_pre_w, NTC, 4);
        for (int l = 0; l < d.NL; ++l) {
            regroup_c(o.enc_w[l], NTC, 3 * KSC);
            regroup_c(o.dec1_w[l], NTC, ((l == 0 && !d.LN) ? KS2 : KSC) + KSC);
            regroup_c(o.dec3_w[l], NTC, 3 * KSC);
        }
        regroup_c(o.post1_w, NTC, 2 * KSC);
        regroup_c(o.post_t_w, 1, KSC);
    }
    *out = std::move(p.v);
    return FE_OK;
}


// The stream-batched per-hop step's scratch of BSRNN / FSPEN / LiSenNet (sb_dev): grow-only, (re)allocated to `bytes` for a batch of
// B >= min_streams streams that is larger than the one it holds (min_streams <= 0: the family's stream-batched step is off).
int ensure_sb_scratch(fe_handle* h, int B, int min_streams, size_t bytes) {
    if (min_streams <= 0 || B < min_streams || B <= h->sb_streams) return FE_OK;
    if (h->sb_dev) { FE_HIP_CHECK(hipFree(h->sb_dev)); h->sb_dev = nullptr; h->sb_streams = 0; }
    FE_HIP_CHECK(hipMalloc(&h->sb_dev, bytes));
    h->sb_streams = B;
    return FE_OK;
}

// One tensor of a streaming state sized for `capacity` streams: [rows][capacity][len] floats, stream-major, `off` floats from the start of
// the state (state_regions lists them; the families' own parts are their traits' regions()).
struct StateRegion {
    size_t off;
    int rows, len;
};
constexpr int kMaxStateRegions = 12;      // (LiSenNet: the two STFT caches + nine model caches)

// frames in flight per stream that the rings of every time pipeline's work buffer are sized for (fe_set_time_pipeline clamps to it)
constexpr int kMaxPipeFrames = 64;

// the baseline families' host sides (weight sections, handle creation, packers, launches, the traits the paths below take): one file each
#include "fe_api_bsrnn.inc"
#include "fe_api_fspen.inc"
#include "fe_api_lisennet.inc"

// The baseline families (BSRNN, FSPEN, LiSenNet) share one implementation of every entry point, parameterised by the family's traits;
// FastEnhancer has paths of its own.  Calls f(Family{}) for a baseline family's arch and returns true; false for FastEnhancer.
template <class F>
bool visit_baseline(int arch, F&& f) {
    switch (arch) {
    case FE_ARCH_BSRNN: f(BsrnnFamily{}); return true;
    case FE_ARCH_FSPEN: f(FspenFamily{}); return true;
    case FE_ARCH_LISENNET: f(LisennetFamily{}); return true;
    default: return false;
    }
}

// what a compute entry point enqueues ends up in its handle (fe_last_step_kernel)
struct KernelLogScope {
    fe_handle* h;
    explicit KernelLogScope(fe_handle* h_) : h(h_) {
        fe::g_klog.n = 0;
        h->last_shape = h->impl ? h->impl->name : nullptr;
        visit_baseline(h->cfg.arch, [&](auto F) { h->last_shape = F.shape_name(h); });
    }
    ~KernelLogScope() {
        if (!h) return;
        h->n_last_kernels = fe::g_klog.n;
        std::memcpy(h->last_kernels, fe::g_klog.name, sizeof(h->last_kernels));
    }
};

int check_ready(const fe_handle* h) {
    if (!h) return fail(FE_ERR_INVALID_ARG, "null handle");
    if (!h->loaded) return fail(FE_ERR_NO_WEIGHTS, "fe_load_weights has not been called");
    return FE_OK;
}

// Scratch for the encoder outputs of shapes that keep them in global memory: one slot per resident WORKGROUP (the
// grid never exceeds max_wgs), allocated once by fe_load_weights - nothing is allocated, freed or synchronised inside
// the compute calls (they can be captured into HIP graphs).  The slots belong to the handle: launches of one handle
// must be stream-ordered (one stream, or event-ordered streams); concurrent launches need one handle each.
int ensure_scratch(fe_handle* h, int) {
    // (BSRNN: band-LSTM input projections of the C = 64 shape; FastEnhancer: the larger of the shape's own plan and its
    // low-LDS companion's, which runs two workgroups per CU)
    size_t floats = 0;
    if (!visit_baseline(h->cfg.arch, [&](auto F) { floats = F.xp_floats(h); })) {
        floats = (size_t)h->max_wgs * h->impl->occ * h->impl->skip_floats;
        if (h->impl_many) floats = std::max(floats, (size_t)h->max_wgs * h->impl_many->occ * h->impl_many->skip_floats);
    }
    if (floats == 0 || h->skip_dev) return FE_OK;
    FE_HIP_CHECK(hipMalloc(&h->skip_dev, floats * sizeof(float)));
    FE_HIP_CHECK(hipMemset(h->skip_dev, 0, floats * sizeof(float)));
    h->skip_streams = h->max_wgs;
    return FE_OK;
}

// the handle's part of a frame-kernel argument block (a: the fields the caller has set already)
fe::StreamFrameArgs base_args(fe_handle* h, int B, int T, fe::StreamFrameArgs a = {}) {
    a.wp = h->packed_dev;
    a.B = B;
    a.T = T;
    a.compression = h->cfg.input_compression;
    a.rf_eps = h->cfg.rf_eps > 0.0f ? h->cfg.rf_eps : 1.0e-5f;
    a.skip = h->skip_dev;
    a.step_kernel = h->step_kernel;
    return a;
}

}  // namespace

static int ensure_tables(fe_handle* h, hipStream_t st);

// fe_spec_step on the time pipeline for the variants whose frames exchange more than the GRU state (r4v).  dptransformer: the caller's K / V
// caches - per (cache, stream, pair) a ring of L slots whose oldest frame sits in slot `head` of the stream - are laid out as the pipeline's
// rings of RS = L + P slots (ring index j = window position j, oldest first; frame t of the chunk lives at index L + t), and after the
// launch the chunk's last L frames (ring indices T .. T + L - 1) go back to the caller's caches in the reference's order (head = 0): what
// ONNXModel.forward returns (dptransformer/model.py:231-232).  time_kernel: the same for the causal convs' input caches (L = KT - 1 slots of
// [F1][C1] per (conv, stream), no head; time_kernel/model.py:119-148).
// caches [ROWS][L][SZ], rings [ROWS][RS][SZ], ROWS = caches x streams x PAIRS; heads [B] (floats) or nullptr; one thread per float.
__global__ void ring_in_kernel(const float* __restrict__ cache, const float* __restrict__ heads, float* __restrict__ ring, size_t n, int B, int PAIRS,
                               int SZ, int L, int RS) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int dd = (int)(i % SZ);
    const int j = (int)((i / SZ) % L);                // window position, oldest first
    const size_t row = i / ((size_t)SZ * L);
    int slot = j;
    if (heads != nullptr) {
        slot += (int)heads[(row / PAIRS) % B];
        slot = slot >= L ? slot - L : slot;
    }
    ring[(row * RS + j) * SZ + dd] = cache[(row * L + slot) * SZ + dd];
}

__global__ void ring_out_kernel(const float* __restrict__ ring, float* __restrict__ cache, float* __restrict__ heads, size_t n, int B, int SZ, int L, int RS,
                                int T) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (heads != nullptr && i < (size_t)B) heads[i] = 0.0f;
    if (i >= n) return;
    const int dd = (int)(i % SZ);
    const int j = (int)((i / SZ) % L);
    const size_t row = i / ((size_t)SZ * L);
    cache[(row * L + j) * SZ + dd] = ring[(row * RS + (size_t)((T + j) % RS)) * SZ + dd];
}

// fe_debug_poison_lds: every workgroup fills 160 KiB of LDS (= one workgroup per CU at a time) with quiet-NaN patterns; 16 x #CUs workgroups so that every CU
// gets at least one whatever the dispatch order
__global__ void __launch_bounds__(256) poison_lds_kernel(unsigned int* sink) {
    extern __shared__ __attribute__((aligned(16))) unsigned int pl[];
    for (int i = threadIdx.x; i < 160 * 1024 / 4; i += 256) pl[i] = 0x7fc00000u | (unsigned int)i;
    __syncthreads();
    if (pl[(threadIdx.x * 97 + blockIdx.x) % (160 * 1024 / 4)] == 0x12345u && sink) sink[0] = 1u;      // (keeps the stores alive)
}

constexpr size_t round4(size_t n) { return (n + 3) & ~(size_t)3; }

// the overlap-add of windowed frames [B][T][N] into wav_out (rows of out_stride samples; Tw_b: a ragged batch's lengths)
static int ola(fe_handle* h, const float* frames, float* wav_out, size_t out_stride, int B, int T, hipStream_t st, const int* Tw_b = nullptr) {
    const int n_out = h->d.HOP * (T - 1);
    fe::note_kernel("istft_ola_kernel");
    hipLaunchKernelGGL(fe::istft_ola_kernel, dim3((n_out + fe::kThreads - 1) / fe::kThreads, B), dim3(fe::kThreads), 0, st,
                       frames, h->tables_dev, wav_out, out_stride, h->d.NFFT, h->d.HOP, T, Tw_b);
    const hipError_t e = hipGetLastError();
    return launch_rc(e);
}

// The work buffers of the time pipeline: like state_layout() for the streaming state, one function lays each buffer out, and both its
// *_work_floats query and its entry point call it.  The pipeline's own region, in floats from its start: frame counters [rows][counters]
// (at 0; rounded up to 4 floats) | windowed frames [rows][T][N] | the rings of the frames in flight (ring_floats; 0 for variants without).
struct PipeLayout { size_t frames, ring, total; };
static PipeLayout pipe_layout(const fe_handle* h, size_t rows, int T, size_t counters, size_t ring_floats) {
    const size_t frames = round4(rows * counters), ring = frames + rows * T * h->d.NFFT;
    return {frames, ring, ring + ring_floats};
}

// fe_offline on the frame walk: overlap-add tail [B][N-H] (at 0) | the model's state (state_floats) | the pipeline's region p.  The call
// zeroes the first `pipe` floats for the serial walk, pipe + p.frames - the counters too - for the pipelined launch.
struct OfflineLayout { size_t state, pipe; PipeLayout p; size_t total; };
static OfflineLayout offline_layout(const fe_handle* h, int B, int T, size_t state_floats, size_t counters, size_t ring_floats) {
    const size_t state = (size_t)B * (h->d.NFFT - h->d.HOP), pipe = state + state_floats;
    const PipeLayout p = pipe_layout(h, B, T, counters, ring_floats);
    return {state, pipe, p, pipe + p.total};
}

// The pipelined form of a launch: a COPY of the serial walk's argument block, pointed at the pipeline's region.  The caller keeps its own
// block and, where the runtime refuses the cooperative launch, walks with it as it is.
template <class Args>
Args pipe_args(Args a, float* region, const PipeLayout& L, int P) {
    a.pipe_flags = reinterpret_cast<unsigned int*>(region);
    a.frames = region + L.frames;
    a.pipe_p = P;
    return a;
}

// a cooperative launch the runtime refused (no co-residency: GPU shared with other work) leaves its error behind: cleared here
static bool coop_refused(hipError_t e) {
    if (e != hipSuccess) (void)hipGetLastError();
    return e != hipSuccess;
}

// A baseline family's fe_offline work buffer (the state rounded up to 4 floats; the ring is Family::ring_floats per utterance).
// fe_offline_work_floats sizes it for the time-pipelined launch whatever fe_set_time_pipeline says at the time of that call.
template <class Fam>
OfflineLayout baseline_layout(Fam, const fe_handle* h, int B, int T) {
    return offline_layout(h, B, T, round4(Fam::state_floats(h, B)), Fam::counters(h), (size_t)B * Fam::ring_floats(h));
}

// frames in flight per utterance of a baseline family's time-pipelined offline launch (0: one workgroup walks the frames of an utterance)
template <class Fam>
int baseline_pipe_width(Fam, const fe_handle* h, int B, int T) {
    if (!Fam::impl(h)->launch_pipe || h->pipe_frames == 0 || h->pipe_frames == 1 || T < 4) return 0;
    int p = (h->max_wgs * Fam::impl(h)->occ) / B;
    const int want = h->pipe_frames < 0 ? Fam::kPipeFrames : h->pipe_frames;
    p = p < want ? p : want;
    p = p < T ? p : T;
    return p >= 2 ? p : 0;
}

template <class Fam>
int baseline_offline(Fam, fe_handle* h, const float* noisy_dev, int B, int Tw, float* wav_hat_dev, float* spec_hat_dev, float* work_dev, hipStream_t st) {
    const Dims& d = h->d;
    const int T = 1 + Tw / d.HOP;
    const OfflineLayout L = baseline_layout(Fam{}, h, B, T);
    FE_HIP_CHECK(hipMemsetAsync(work_dev, 0, (L.pipe + L.p.frames) * sizeof(float), st));      // (the counters too, whichever launch follows)
    typename Fam::StreamArgs a = Fam::args(h, B, T);
    a.mode = fe::FE_MODE_OFFLINE;
    a.Tw = Tw;
    a.wav_in = noisy_dev; a.in_stride = (size_t)Tw;
    a.wav_out = wav_hat_dev; a.out_stride = (size_t)d.HOP * (T - 1);
    a.spec_out = spec_hat_dev;
    a.cache_istft = work_dev; a.cache_stft = work_dev;
    Fam::state(a) = work_dev + L.state;
    if (const int P = baseline_pipe_width(Fam{}, h, B, T)) {
        // the frames of an utterance over P co-resident workgroups (the family's PIPE kernel); refused co-residency: the serial walk
        const int rc = ensure_tables(h, st);
        if (rc != FE_OK) return rc;
        typename Fam::Args p = pipe_args(a, work_dev + L.pipe, L.p, P);
        Fam::set_ring(p, work_dev + L.pipe + L.p.ring);
        hipError_t e = hipSuccess;
        Fam::impl(h)->launch_pipe(p, st, &e);
        if (!coop_refused(e)) return ola(h, p.frames, wav_hat_dev, a.out_stride, B, T, st);
    }
    return Fam::launch_step(h, a, fe::STEP_PLAIN, st);
}

extern "C" {

int fe_debug_poison_lds(void* stream) {
    int dev = 0, cus = 0;
    FE_HIP_CHECK(hipGetDevice(&dev));
    FE_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    FE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&poison_lds_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    hipLaunchKernelGGL(poison_lds_kernel, dim3(16 * (cus > 0 ? cus : 256)), dim3(256), 160 * 1024, (hipStream_t)stream, (unsigned int*)nullptr);
    FE_HIP_CHECK(hipGetLastError());
    return FE_OK;
}

const char* fe_last_error(void) { return g_err.c_str(); }
const char* fe_version(void) { return "fastenhancer_hip 0.1 (gfx950)"; }

int fe_create(const fe_config* cfg, fe_handle** out) {
    if (!cfg || !out) return fail(FE_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    int rc = FE_OK;
    if (visit_baseline(cfg->arch, [&](auto F) { rc = F.create(cfg, out); })) return rc;
    if (cfg->arch != FE_ARCH_FASTENHANCER)
        return fail(FE_ERR_UNSUPPORTED_CONFIG, "arch %d is not built into this library", cfg->arch);
    if (cfg->n_fft % 2 != 0) return fail(FE_ERR_INVALID_ARG, "`n_fft` must be an even number, but given %d.", cfg->n_fft);
    if (cfg->win_size > cfg->n_fft) return fail(FE_ERR_INVALID_ARG, "n_fft(%d) must be bigger than win_size(%d)", cfg->n_fft, cfg->win_size);
    if (cfg->hop_size <= 0 || cfg->hop_size > cfg->n_fft) return fail(FE_ERR_INVALID_ARG, "hop_size %d out of range", cfg->hop_size);
    if (cfg->stride != 4) return fail(FE_ERR_UNSUPPORTED_CONFIG, "stride %d (every shipped config uses 4)", cfg->stride);
    if (cfg->n_kernels < 2 || cfg->n_kernels > FE_MAX_KERNELS) return fail(FE_ERR_INVALID_ARG, "len(kernel_size)=%d", cfg->n_kernels);
    if (cfg->kernel_size[0] != 8) return fail(FE_ERR_UNSUPPORTED_CONFIG, "kernel_size[0]=%d (shipped: 8)", cfg->kernel_size[0]);
    for (int i = 1; i < cfg->n_kernels; ++i)
        if (cfg->kernel_size[i] != 3) return fail(FE_ERR_UNSUPPORTED_CONFIG, "kernel_size[%d]=%d (shipped: 3)", i, cfg->kernel_size[i]);
    if (cfg->rf_heads != 4) return fail(FE_ERR_UNSUPPORTED_CONFIG, "num_heads=%d (shipped: 4)", cfg->rf_heads);
    if (!(cfg->input_compression > 0.0f && cfg->input_compression <= 1.0f)) return fail(FE_ERR_INVALID_ARG, "input_compression");

    const fe::Impl* impl = nullptr;
    const int kt = cfg->kernel_size_time > 1 ? cfg->kernel_size_time : 1;
    const int fr = cfg->channels_frnn > 0 ? 1 : 0;
    if (fr && 2 * cfg->channels_frnn != cfg->rf_channels)
        return fail(FE_ERR_UNSUPPORTED_CONFIG, "channels_frnn=%d with channels=%d (the dprnn kernels are built for channels_frnn = channels / 2, every shipped yaml)",
                    cfg->channels_frnn, cfg->rf_channels);
    const int ln = cfg->ln ? 1 : 0;
    if (ln && (fr || cfg->lookbehind > 0 || kt > 1)) return fail(FE_ERR_INVALID_ARG, "ln excludes channels_frnn / lookbehind / kernel_size_time");
    const int bd = cfg->bidirectional ? 1 : 0;
    if (bd && (fr || cfg->lookbehind > 0 || kt > 1 || ln)) return fail(FE_ERR_INVALID_ARG, "bidirectional excludes channels_frnn / lookbehind / kernel_size_time / ln");
    const int ta = cfg->lookbehind > 0 ? cfg->lookbehind : 0;
    if (ta && ta != 31) return fail(FE_ERR_UNSUPPORTED_CONFIG, "lookbehind=%d (the dptransformer kernels are built for 31, every shipped yaml)", ta);
    if (ta && fr) return fail(FE_ERR_INVALID_ARG, "channels_frnn and lookbehind are exclusive");
    // constructor options beyond the shipped yamls (models/fastenhancer/default/model.py:384-419): compiled per shape as Shape::EP
    if (cfg->activation < FE_ACT_SILU || cfg->activation > FE_ACT_GELU_TANH) return fail(FE_ERR_INVALID_ARG, "activation=%d (FE_ACT_*)", cfg->activation);
    if (cfg->mask < FE_MASK_NONE || cfg->mask > FE_MASK_TANH) return fail(FE_ERR_INVALID_ARG, "mask=%d (FE_MASK_*)", cfg->mask);
    if (cfg->resnet) return fail(FE_ERR_UNSUPPORTED_CONFIG, "resnet=1 is not built into this library (every shipped yaml uses resnet: false)");
    const int ep = cfg->activation + 8 * cfg->mask;
    if (ep && (fr || ta || bd))
        return fail(FE_ERR_UNSUPPORTED_CONFIG, "activation=%d / mask=%d: the options are built for the default, time_kernel and ln models only (this is the %s variant)",
                    cfg->activation, cfg->mask, fr ? "dprnn" : (ta ? "dptransformer" : "noncausal"));
    static const char* const act_names[] = {"silu", "relu", "leaky_relu", "elu", "gelu", "gelu_tanh"};
    static const char* const mask_names[] = {"none", "sigmoid", "tanh"};
    char ep_arg[64] = "";
    if (ep) snprintf(ep_arg, sizeof ep_arg, ",act=%s,mask=%s", act_names[cfg->activation], mask_names[cfg->mask]);
    for (const fe::Impl* im : impls())
        if (im->C1 == cfg->channels && im->NL == cfg->n_kernels - 1 && im->C2 == cfg->rf_channels && im->F2 == cfg->rf_freq &&
            im->KB == cfg->rf_blocks && im->NFFT == cfg->n_fft && im->HOP == cfg->hop_size && im->KT == kt && im->LOW == 0 && im->FR == fr && im->TA == ta && im->LN == ln && im->BD == bd &&
            im->EP == ep)
            impl = im;
    const fe::Impl* impl_many = nullptr;
    for (const fe::Impl* im : impls())
        if (impl && im->LOW >= 1 && im->occ >= 2 && im->C1 == impl->C1 && im->NL == impl->NL && im->C2 == impl->C2 && im->F2 == impl->F2 &&
            im->KB == impl->KB && im->NFFT == impl->NFFT && im->HOP == impl->HOP && im->KT == impl->KT && im->FR == impl->FR && im->TA == impl->TA && im->LN == impl->LN && !impl->BD &&
            im->EP == impl->EP)
            impl_many = im;
    // a companion reads its shape's packed buffer: every offset it uses must be the same function of the shape (fe::Pack does not depend on LOW; r4x: the
    // k4 copies sit behind the time-batched engine's and the 512-thread kernel's sections - checked here rather than trusted)
    if (impl && impl_many && (impl_many->off->k4_delta != impl->off->k4_delta || impl_many->off->conv_k4_delta != impl->off->conv_k4_delta ||
                              impl_many->off->window != impl->off->window || impl_many->off->blk_wih[0] != impl->off->blk_wih[0]))
        return fail(FE_ERR_UNSUPPORTED_CONFIG, "build error: the low-LDS companion of this shape was compiled with a different packed-weight layout (fe::Pack must not depend on LOW)");
    if (!impl)
        return fail(FE_ERR_UNSUPPORTED_CONFIG,
                    "no kernel compiled for channels=%d layers=%d rf_channels=%d rf_freq=%d rf_blocks=%d n_fft=%d hop=%d kernel_size_time=%d%s%s%s "
                    "(build it: python -m fastenhancer_amd.build --add-shape %d,%d,%d,%d,%d,%d,%d,%d%s%s)",
                    cfg->channels, cfg->n_kernels - 1, cfg->rf_channels, cfg->rf_freq, cfg->rf_blocks, cfg->n_fft, cfg->hop_size, kt, fr ? " dprnn" : (ta ? " dptransformer" : (ln ? " ln" : (bd ? " noncausal" : ""))),
                    ep_arg[0] ? " " : "", ep_arg[0] ? ep_arg + 1 : "",
                    cfg->channels, cfg->n_kernels - 1, cfg->rf_channels, cfg->rf_freq, cfg->rf_blocks, cfg->n_fft, cfg->hop_size, kt, fr ? ",0,1" : (ta ? ",0,0,31" : (ln ? ",0,0,0,1" : (bd ? ",0,0,0,0,1" : ""))),
                    ep_arg);
    if (impl->lds_bytes > 160 * 1024)
        return fail(FE_ERR_UNSUPPORTED_CONFIG, "shape needs %zu bytes of LDS (> 160 KiB per CU)", impl->lds_bytes);
    Dims d{impl->C1, impl->NL, impl->C2, impl->F2, impl->KB, impl->NFFT, impl->HOP, impl->NFFT / 2, impl->NFFT / 8, impl->C2 / 4, {0}};
    d.KT = impl->KT;
    d.FR = impl->FR;
    d.TA = impl->TA;
    d.LN = impl->LN;
    d.BD = impl->BD;
    for (int i = 0; i < cfg->n_kernels; ++i) d.ks[i] = cfg->kernel_size[i];
    fe_handle* h = new_handle(cfg, d);
    h->impl = impl;
    h->impl_many = impl_many;              // (fe_set_option("low_lds_companion", 0) keeps run_step off it)
    build_sections(h);
    *out = h;
    return FE_OK;
}

void fe_destroy(fe_handle* h) {
    if (!h) return;
    if (h->packed_dev) (void)hipFree(h->packed_dev);
    if (h->skip_dev) (void)hipFree(h->skip_dev);
    if (h->tables_dev) (void)hipFree(h->tables_dev);
    if (h->pipe_flags_dev) (void)hipFree(h->pipe_flags_dev);
    if (h->tb_probe_dev) (void)hipFree(h->tb_probe_dev);
    if (h->tb_work_dev) (void)hipFree(h->tb_work_dev);
    if (h->spec_ring_dev) (void)hipFree(h->spec_ring_dev);
    if (h->sb_dev) (void)hipFree(h->sb_dev);
    if (h->bsync_dev) (void)hipFree(h->bsync_dev);
    for (hipStream_t s : h->host_streams) if (s) (void)hipStreamDestroy(s);
    for (hipEvent_t e : h->host_events) if (e) (void)hipEventDestroy(e);
    if (h->ident_slots_dev) (void)hipFree(h->ident_slots_dev);
    delete h;
}

#ifdef FE_TB_PROBE
// probe builds only (not part of the ABI): read and clear the time-batched engine's phase clocks, out[4 * kProbeSlots]
extern "C" int fe_tb_probe_read(fe_handle* h, unsigned long long* out) {
    if (!h || !h->tb_probe_dev) return FE_ERR_INVALID_ARG;
    FE_HIP_CHECK(hipDeviceSynchronize());
    FE_HIP_CHECK(hipMemcpy(out, h->tb_probe_dev, 4 * fe::tb::kProbeSlots * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    FE_HIP_CHECK(hipMemset(h->tb_probe_dev, 0, 4 * fe::tb::kProbeSlots * sizeof(unsigned long long)));
    return FE_OK;
}
#endif

size_t fe_weight_floats(const fe_handle* h) { return h ? h->blob_floats : 0; }
int fe_weight_sections(const fe_handle* h) { return h ? (int)h->sections.size() : 0; }

int fe_weight_section(const fe_handle* h, int idx, const char** name, size_t* offset_floats, size_t* count_floats) {
    if (!h || idx < 0 || idx >= (int)h->sections.size()) return fail(FE_ERR_INVALID_ARG, "section index %d", idx);
    if (name) *name = h->sections[idx].name.c_str();
    if (offset_floats) *offset_floats = h->sections[idx].offset;
    if (count_floats) *count_floats = h->sections[idx].count;
    return FE_OK;
}

// the one packing path: fused blob (host) -> the buffer the kernels read (host); no HIP call
static int pack_blob(fe_handle* h, const float* blob, std::vector<float>* packed) {
    int rc = FE_OK;
    const Blob S{h, blob};
    if (!visit_baseline(h->cfg.arch, [&](auto F) { rc = F.pack_weights(h, S, packed); })) rc = pack_weights(h, S, packed);
    return rc;
}

int fe_debug_pack_weights(fe_handle* h, const float* blob_host, size_t nfloats, float* out_host, size_t capacity, size_t* packed_floats) {
    if (!h || !blob_host) return fail(FE_ERR_INVALID_ARG, "null argument");
    if (nfloats != h->blob_floats) return fail(FE_ERR_INVALID_ARG, "blob has %zu floats, expected %zu", nfloats, h->blob_floats);
    std::vector<float> packed;
    const int rc = pack_blob(h, blob_host, &packed);
    if (rc != FE_OK) return rc;
    if (out_host && capacity < packed.size()) return fail(FE_ERR_INVALID_ARG, "output holds %zu floats, the packed buffer has %zu", capacity, packed.size());
    if (packed_floats) *packed_floats = packed.size();
    if (out_host) std::memcpy(out_host, packed.data(), packed.size() * sizeof(float));
    return FE_OK;
}

// the families fe_set_weight_banks(n > 1) serves: FastEnhancer's streaming models (what the packet step runs); else the family's name
static const char* banks_unsupported(const fe_handle* h) {
    switch (h->cfg.arch) {
    case FE_ARCH_BSRNN: return "BSRNN";
    case FE_ARCH_FSPEN: return "FSPEN";
    case FE_ARCH_LISENNET: return "LiSenNet";
    default: return h->d.BD ? "noncausal FastEnhancer" : nullptr;
    }
}

int fe_weight_banks(const fe_handle* h) { return h ? h->n_banks : 0; }

int fe_set_weight_banks(fe_handle* h, int n_banks, void* stream) {
    if (!h) return fail(FE_ERR_INVALID_ARG, "null handle");
    if (n_banks < 1 || n_banks > FE_MAX_WEIGHT_BANKS)
        return fail(FE_ERR_INVALID_ARG, "fe_set_weight_banks: n_banks %d outside [1, FE_MAX_WEIGHT_BANKS = %d]", n_banks, FE_MAX_WEIGHT_BANKS);
    if (n_banks > 1)
        if (const char* family = banks_unsupported(h))
            return fail(FE_ERR_UNSUPPORTED_CONFIG, "fe_set_weight_banks: weight banks are built for the FastEnhancer streaming models (default, time_kernel, ln, "
                        "dprnn, dptransformer), which fe_step_streams_banked steps; this is a %s handle (one bank)", family);
    if (n_banks == h->n_banks) return FE_OK;
    if (h->packed_dev) {      // the banks that survive move to an allocation of the new size; every launch that reads the old one has completed before it goes
        const size_t keep = (size_t)std::min(n_banks, h->n_banks) * h->bank_stride;
        float* fresh = nullptr;
        FE_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
        FE_HIP_CHECK(hipMalloc(&fresh, (size_t)n_banks * h->bank_stride * sizeof(float)));
        hipError_t e = hipMemset(fresh, 0, (size_t)n_banks * h->bank_stride * sizeof(float));
        if (e == hipSuccess) e = hipMemcpy(fresh, h->packed_dev, keep * sizeof(float), hipMemcpyDeviceToDevice);
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e != hipSuccess) { (void)hipFree(fresh); return fail(FE_ERR_HIP, "fe_set_weight_banks: %s", hipGetErrorString(e)); }
        float* old = h->packed_dev;
        h->packed_dev = fresh;         // (the handle owns the new allocation whatever the free of the old one says)
        h->bank_loaded.resize((size_t)n_banks, 0);
        h->n_banks = n_banks;
        FE_HIP_CHECK(hipFree(old));
        return FE_OK;
    }
    h->bank_loaded.resize((size_t)n_banks, 0);
    h->n_banks = n_banks;
    return FE_OK;
}

int fe_load_weights_bank(fe_handle* h, int bank, const float* blob_dev, size_t nfloats, void* stream) {
    if (!h || !blob_dev) return fail(FE_ERR_INVALID_ARG, "null argument");
    if (bank < 0 || bank >= h->n_banks) return fail(FE_ERR_INVALID_ARG, "bank %d outside [0, %d) (fe_set_weight_banks)", bank, h->n_banks);
    if (nfloats != h->blob_floats) return fail(FE_ERR_INVALID_ARG, "blob has %zu floats, expected %zu", nfloats, h->blob_floats);
    hipStream_t st = (hipStream_t)stream;
    std::vector<float> blob(nfloats);
    FE_HIP_CHECK(hipMemcpyAsync(blob.data(), blob_dev, nfloats * sizeof(float), hipMemcpyDeviceToHost, st));
    FE_HIP_CHECK(hipStreamSynchronize(st));
    std::vector<float> packed;
    int rc = pack_blob(h, blob.data(), &packed);
    if (rc != FE_OK) return rc;
    const size_t stride = (packed.size() + 63) & ~(size_t)63;
    if (h->packed_dev && h->n_banks == 1 && stride != h->bank_stride) { FE_HIP_CHECK(hipFree(h->packed_dev)); h->packed_dev = nullptr; }
    if (h->packed_dev && stride != h->bank_stride) return fail(FE_ERR_INVALID_ARG, "packed buffer of %zu floats in banks of %zu", packed.size(), h->bank_stride);
    if (h->packed_dev && h->n_banks == 1) FE_HIP_CHECK(hipDeviceSynchronize());      // (a one-bank handle's load waits for every launch that reads the buffer, as it always has)
    if (!h->packed_dev) {     // the first load of the handle allocates all banks; later loads write their bank in place
        FE_HIP_CHECK(hipMalloc(&h->packed_dev, (size_t)h->n_banks * stride * sizeof(float)));
        FE_HIP_CHECK(hipMemsetAsync(h->packed_dev, 0, (size_t)h->n_banks * stride * sizeof(float), st));
        h->bank_stride = stride;
    }
    FE_HIP_CHECK(hipMemcpyAsync(h->packed_dev + (size_t)bank * stride, packed.data(), packed.size() * sizeof(float), hipMemcpyHostToDevice, st));
    FE_HIP_CHECK(hipStreamSynchronize(st));
    rc = ensure_scratch(h, 0);
    if (rc != FE_OK) return rc;
    h->bank_loaded[(size_t)bank] = 1;
    if (bank == 0) h->loaded = true;
    return FE_OK;
}

int fe_load_weights(fe_handle* h, const float* blob_dev, size_t nfloats, void* stream) { return fe_load_weights_bank(h, 0, blob_dev, nfloats, stream); }

// time_kernel variant: floats of the causal convs' frame caches per stream (2 NL layers x [KT-1][F1][C1])
static size_t tk_floats(const fe_handle* h) {
    const Dims& d = h->d;
    return (size_t)2 * d.NL * (d.KT - 1) * d.F1 * d.C1;
}

// The streaming state of `rows` streams, in floats from its start: cache_stft [rows][N-H] at 0, cache_istft [rows][N-H], then the model's
// own state - FastEnhancer: h (GRU states or K / V rings, rows * hstate()), tk (the time_kernel conv caches), total floats; the other
// families lay out their own state from h on.  rows = B for fe_step, the capacity for the slotted entry points.
struct StateLayout { size_t cache_istft, h, tk, total; };
static StateLayout state_layout(const fe_handle* h, size_t rows) {
    const size_t ovl = (size_t)(h->d.NFFT - h->d.HOP), hs = 2 * rows * ovl, tk = hs + rows * h->d.hstate();
    return {rows * ovl, hs, tk, tk + rows * tk_floats(h)};
}

size_t fe_state_floats(const fe_handle* h, int B) {
    if (!h || B <= 0) return 0;
    size_t n = 0;
    if (visit_baseline(h->cfg.arch, [&](auto F) { n = state_layout(h, B).h + F.state_floats(h, B); })) return n;
    return state_layout(h, B).total;
}

int fe_state_init(fe_handle* h, float* state_dev, int B, void* stream) {
    if (!h || !state_dev || B <= 0) return fail(FE_ERR_INVALID_ARG, "bad argument");
    FE_HIP_CHECK(hipMemsetAsync(state_dev, 0, fe_state_floats(h, B) * sizeof(float), (hipStream_t)stream));
    // (the scratch of the stream-batched per-hop step: sized here, so that the steps of this batch allocate nothing)
    int rc = FE_OK;
    visit_baseline(h->cfg.arch, [&](auto F) { rc = F.ensure_sb(h, B); });
    return rc;
}

static const char* const kNoncausalNoStep =
    "the noncausal model has no streaming step (models/fastenhancer/noncausal/model.py has the offline Model only): use fe_offline";

// FastEnhancer's streaming step of B streams: the shape's own record, or - per-hop launches above the streams the shape's own plan holds at once
// (#CUs; 2 x #CUs for T) - the low-LDS companion (two workgroups per CU, three for the T shapes; same packed weights - Pack<S> does not depend
// on LOW), where one is compiled and measured faster.  probe: a debug / profile step (always the shape's own record)
static const fe::Impl* step_impl(const fe_handle* h, int B, int T, bool probe) {
    if (h->impl_many && h->opt[OPT_LOW_LDS_COMPANION] && T == 1 && B > h->max_wgs * h->impl->occ && (h->impl_many->many_persist || B <= h->max_wgs * h->impl_many->occ) &&
        (h->impl_many->many_one_round || B > h->max_wgs * h->impl_many->occ) && !probe &&
        !(h->step_kernel == FE_STEP_KERNEL_WG8_PERSIST && h->impl->wg8))
        return h->impl_many;
    return h->impl;
}

// the slotted entry points: FastEnhancer's causal models only (checked after the handle and before the arguments' contents)
static int check_slots_family(const fe_handle* h, const char* fn) {
    if (h->cfg.arch != FE_ARCH_FASTENHANCER)
        return fail(FE_ERR_UNSUPPORTED_CONFIG, "%s: slot-indexed state is built for the FastEnhancer family (the default, time_kernel, ln, dprnn and "
                    "dptransformer models); BSRNN, FSPEN and LiSenNet step whole state buffers with fe_step", fn);
    if (h->d.BD) return fail(FE_ERR_UNSUPPORTED_CONFIG, "%s", kNoncausalNoStep);
    return FE_OK;
}

// "audio in, audio out, state, count, T, strides" of every streaming step.  ptrs: all pointers of the call are non-null; capacity = n for the
// steps without a slot list.  fn (the pinned steps name themselves; else nullptr) and bad (the wording of the first refusal) are the entry point's own.
static int check_step_args(const fe_handle* h, const char* fn, const char* bad, bool ptrs, int n, int capacity, int T, size_t in_stride, size_t out_stride) {
    const char* sep = fn ? ": " : "";
    if (!fn) fn = "";
    if (!ptrs || n <= 0 || T <= 0 || capacity < n) return fail(FE_ERR_INVALID_ARG, "%s%s%s", fn, sep, bad);
    const size_t row = (size_t)T * h->d.HOP;
    if (in_stride < row && n > 1) return fail(FE_ERR_INVALID_ARG, "%s%sin_stride %zu < T*H", fn, sep, in_stride);
    if (out_stride < row && n > 1) return fail(FE_ERR_INVALID_ARG, "%s%sout_stride %zu < T*H", fn, sep, out_stride);
    return FE_OK;
}
static const char* const kBadSlotArgs = "bad argument (need non-null pointers, 1 <= n <= capacity, T >= 1)";

// What a streaming step of any family puts into its argument block for the call: streaming mode, audio pointers and strides, and the two STFT caches
// at the head of a state of L's rows.  Returns where the model's own state starts (L.h).
extern "C++" template <class Args>
static float* stream_io(Args& a, const float* wav_in, size_t in_stride, float* wav_out, size_t out_stride, float* state, const StateLayout& L) {
    a.mode = fe::FE_MODE_STREAM;
    a.wav_in = wav_in; a.wav_out = wav_out; a.in_stride = in_stride; a.out_stride = out_stride;
    a.cache_stft = state; a.cache_istft = state + L.cache_istft;
    return state + L.h;
}

// FastEnhancer's streaming step of n streams, however it was asked for: the entry point sets the flavour's own fields in `own`, this fills in the
// rest and launches.  own.capacity = the rows of the state (n for the plain flavour).  STEP_PLAIN (fe_step, the debug / profile steps): dbg, clk,
// dbg_stride.  STEP_SLOTS / STEP_SLOTS_PINNED: slots - the launch fe_step(B = n) makes with every state address taken from (slots[b], capacity);
// pinned: wav_in / wav_out are device views of page-locked host memory.  STEP_STREAMS: desc, in_count, out_count, format, pinned (no strides).
static fe::StreamFrameArgs fe_step_args(fe_handle* h, const fe::StreamFrameArgs& own, const float* wav_in, size_t in_stride, float* state, float* wav_out,
                                        size_t out_stride, int n, int T) {
    fe::StreamFrameArgs a = base_args(h, n, T, own);
    const StateLayout L = state_layout(h, own.capacity);
    a.h = stream_io(a, wav_in, in_stride, wav_out, out_stride, state, L);
    a.tk = state + L.tk;
    return a;
}

static int launch_fe_step(fe_handle* h, const char* fn, fe::StepFlavour flavour, const fe::StreamFrameArgs& own, const float* wav_in, size_t in_stride,
                          float* state, float* wav_out, size_t out_stride, int n, int T, void* stream) {
    int rc = ensure_scratch(h, n);
    if (rc != FE_OK) return rc;
    fe::StreamFrameArgs a = fe_step_args(h, own, wav_in, in_stride, state, wav_out, out_stride, n, T);
    const fe::Impl* im = step_impl(h, n, T, a.dbg || a.clk);
    if (!im->launch_step) {      // (a noncausal record; every entry point refuses those models earlier.  The slotted wording names the entry point's family, not fn, as it always has)
        const char* shape = im->name ? im->name : "?";
        if (flavour == fe::STEP_PLAIN) return fail(FE_ERR_UNSUPPORTED_CONFIG, "%s", kNoncausalNoStep);
        if (flavour == fe::STEP_STREAMS) return fail(FE_ERR_UNSUPPORTED_CONFIG, "%s: no packet-audio kernel is compiled for shape %s", fn, shape);
        return fail(FE_ERR_UNSUPPORTED_CONFIG, "%s: no slotted kernel is compiled for shape %s", flavour == fe::STEP_SLOTS_PINNED ? "fe_step_slots_pinned" : "fe_step_slots", shape);
    }
    h->last_shape = im->name;
    hipError_t e = hipSuccess;
    im->launch_step(a, flavour, h->max_wgs, (hipStream_t)stream, &e);
    return launch_rc(e);
}

// launch_fe_step's counterpart for BSRNN, FSPEN and LiSenNet: the family's streaming step of n streams, however it was asked for.  The entry point
// sets the flavour's own fields in `own`, this builds the family's argument block around them and launches.  own.capacity = the rows of the state
// (n for the plain flavour).  STEP_PLAIN (fe_step, the debug / profile steps): dbg, clk.  STEP_SLOTS (fe_step_pool): slots.  STEP_STREAMS
// (fe_step_pool_streams[_pinned]): io - desc, in_count, out_count, format, pinned (no strides: each stream's rows lie at its own offsets).
struct BaselineStepOwn {
    float* dbg = nullptr;
    unsigned long long* clk = nullptr;
    int capacity = 0;
    const int* slots = nullptr;
    fe::StreamIoArgs io{};
};
static int launch_baseline_step(fe_handle* h, fe::StepFlavour flavour, const BaselineStepOwn& own, const float* wav_in, size_t in_stride, float* state,
                                float* wav_out, size_t out_stride, int n, int T, void* stream) {
    int rc = FE_OK;
    visit_baseline(h->cfg.arch, [&](auto F) {
        auto a = F.args(h, n, T);
        if (flavour == fe::STEP_PLAIN) { a.dbg = own.dbg; a.clk = own.clk; a.dbg_stride = F.impl(h)->dbg_floats; }
        a.capacity = own.capacity;
        a.slots = own.slots;
        static_cast<fe::StreamIoArgs&>(a) = own.io;
        F.state(a) = stream_io(a, wav_in, in_stride, wav_out, out_stride, state, state_layout(h, own.capacity));
        rc = F.launch_step(h, a, flavour, stream);
    });
    return rc;
}

static int run_step(fe_handle* h, const float* wav_in, size_t in_stride, float* state, float* wav_out, size_t out_stride,
                    int B, int T, float* dbg, unsigned long long* clk, void* stream) {
    int rc = check_ready(h);
    if (rc != FE_OK) return rc;
    KernelLogScope klog_(h);
    rc = check_step_args(h, nullptr, "bad argument", wav_in && state && wav_out, B, B, T, in_stride, out_stride);
    if (rc != FE_OK) return rc;
    if (h->cfg.arch != FE_ARCH_FASTENHANCER) {
        BaselineStepOwn own;
        own.dbg = dbg; own.clk = clk;
        own.capacity = B;
        return launch_baseline_step(h, fe::STEP_PLAIN, own, wav_in, in_stride, state, wav_out, out_stride, B, T, stream);
    }
    if (h->d.BD) return fail(FE_ERR_UNSUPPORTED_CONFIG, "%s", kNoncausalNoStep);
    fe::StreamFrameArgs own{};
    own.dbg = dbg; own.clk = clk; own.dbg_stride = h->impl->dbg_floats;
    own.capacity = B;
    return launch_fe_step(h, "fe_step", fe::STEP_PLAIN, own, wav_in, in_stride, state, wav_out, out_stride, B, T, stream);
}

int fe_step(fe_handle* h, const float* wav_in_dev, size_t in_stride, float* state_dev, float* wav_out_dev, size_t out_stride,
            int B, int T, void* stream) {
    return run_step(h, wav_in_dev, in_stride, state_dev, wav_out_dev, out_stride, B, T, nullptr, nullptr, stream);
}

// What every slotted entry point does before it enqueues anything: handle, family, the call's own arguments (check_args), the handle's readiness; go()
// then runs inside the kernel log's scope.  args_first: the pinned and packet steps check their arguments before readiness and outside that scope,
// fe_step_slots after it and inside (a refused call empties fe_last_step_kernel's answer) - which of two faults a call reports depends on this order:
// deliberate API history, pinned by tests/test_c_abi_errors.py.
extern "C++" template <class Check, class Go>
static int slotted_step(fe_handle* h, const char* fn, bool args_first, Check&& check_args, Go&& go) {
    if (!h) return fail(FE_ERR_INVALID_ARG, "null handle");
    int rc = check_slots_family(h, fn);
    if (rc == FE_OK && args_first) rc = check_args();
    if (rc == FE_OK) rc = check_ready(h);
    if (rc != FE_OK) return rc;
    KernelLogScope klog_(h);
    if (!args_first) rc = check_args();
    return rc != FE_OK ? rc : go();
}

int fe_step_slots(fe_handle* h, const float* wav_in_dev, size_t in_stride, float* state_dev, int capacity, const int* slots_dev,
                  float* wav_out_dev, size_t out_stride, int n, int T, void* stream) {
    return slotted_step(h, "fe_step_slots", false,
        [&] { return check_step_args(h, nullptr, kBadSlotArgs, wav_in_dev && state_dev && slots_dev && wav_out_dev, n, capacity, T, in_stride, out_stride); },
        [&] {
            fe::StreamFrameArgs own{};
            own.capacity = capacity; own.slots = slots_dev;
            return launch_fe_step(h, "fe_step_slots", fe::STEP_SLOTS, own, wav_in_dev, in_stride, state_dev, wav_out_dev, out_stride, n, T, stream);
        });
}

// fe_step_pool: fe_step_slots for every family with a streaming state.  FastEnhancer's handles take fe_step_slots' path as it stands (the noncausal
// model its refusal, which is fe_step's); a baseline family runs the per-stream kernels fe_step(B = n, T) picks, in their slotted instantiations,
// with fe_step_slots' checks in fe_step_slots' order.
int fe_step_pool(fe_handle* h, const float* wav_in_dev, size_t in_stride, float* state_dev, int capacity, const int* slots_dev,
                 float* wav_out_dev, size_t out_stride, int n, int T, void* stream) {
    if (!h) return fail(FE_ERR_INVALID_ARG, "null handle");
    if (h->cfg.arch == FE_ARCH_FASTENHANCER)
        return fe_step_slots(h, wav_in_dev, in_stride, state_dev, capacity, slots_dev, wav_out_dev, out_stride, n, T, stream);
    int rc = check_ready(h);
    if (rc != FE_OK) return rc;
    KernelLogScope klog_(h);
    rc = check_step_args(h, nullptr, kBadSlotArgs, wav_in_dev && state_dev && slots_dev && wav_out_dev, n, capacity, T, in_stride, out_stride);
    if (rc != FE_OK) return rc;
    BaselineStepOwn own;
    own.capacity = capacity; own.slots = slots_dev;
    return launch_baseline_step(h, fe::STEP_SLOTS, own, wav_in_dev, in_stride, state_dev, wav_out_dev, out_stride, n, T, stream);
}

// fe_step_pinned / fe_step_slots_pinned: `count` floats from p must be page-locked host memory with a device mapping on the current device
// (hipHostMalloc / hipHostRegister: torch's pin_memory()).  Anything else - pageable or device memory - would make the kernel take a page
// fault, so it is refused here, before any launch.  Both ends of the range are looked up; *dev = the device view of p.
// (E: float, or short for the int16 audio of fe_step_streams_pinned, whose buffers are typed by the call's format - hence void pointers.)
extern "C++" template <class E>
static int pinned_view(const void* p, size_t count, const char* fn, const char* what, const void** dev) {
    const E* ends[2] = {static_cast<const E*>(p), static_cast<const E*>(p) + (count - 1)};
    const char* dv[2] = {nullptr, nullptr};
    for (int i = 0; i < 2; ++i) {
        hipPointerAttribute_t at{};
        bool ok = hipPointerGetAttributes(&at, ends[i]) == hipSuccess && at.type == hipMemoryTypeHost;
        void* dp = nullptr;
        if (ok) ok = hipHostGetDevicePointer(&dp, const_cast<E*>(ends[i]), 0) == hipSuccess && dp != nullptr;
        (void)hipGetLastError();        // (a refused lookup must not surface as the error of a later launch)
        if (!ok)
            return fail(FE_ERR_INVALID_ARG, "%s: %s is not page-locked host memory mapped for this device (%s element of the range): pin the buffer "
                        "(torch: pin_memory(); C: hipHostMalloc / hipHostRegister)", fn, what, i ? "last" : "first");
        dv[i] = static_cast<const char*>(dp);
    }
    if (dv[1] - dv[0] != reinterpret_cast<const char*>(ends[1]) - reinterpret_cast<const char*>(ends[0]))
        return fail(FE_ERR_INVALID_ARG, "%s: %s spans more than one pinned allocation: pin the buffer as one piece (pin_memory())", fn, what);
    *dev = dv[0];
    return FE_OK;
}

// the identity slot list 0 .. B-1 of fe_step_pinned (grow-only; written before the first step that needs it, not inside a capture)
static int ensure_ident_slots(fe_handle* h, int B) {
    if (h->ident_slots >= B) return FE_OK;
    int cap = 256;
    while (cap < B) cap *= 2;
    std::vector<int> ids(cap);
    for (int i = 0; i < cap; ++i) ids[i] = i;
    if (h->ident_slots_dev) { FE_HIP_CHECK(hipFree(h->ident_slots_dev)); h->ident_slots_dev = nullptr; h->ident_slots = 0; }    // (hipFree waits for the launches that read it)
    FE_HIP_CHECK(hipMalloc(&h->ident_slots_dev, cap * sizeof(int)));
    FE_HIP_CHECK(hipMemcpy(h->ident_slots_dev, ids.data(), cap * sizeof(int), hipMemcpyHostToDevice));
    h->ident_slots = cap;
    return FE_OK;
}

// identity: fe_step_pinned (capacity = n, stream i = slot i of the handle's identity list)
static int step_pinned(fe_handle* h, const char* fn, const float* wav_in_host, size_t in_stride, float* state_dev, int capacity, const int* slots_dev,
                       bool identity, float* wav_out_host, size_t out_stride, int n, int T, void* stream) {
    return slotted_step(h, fn, true,
        [&] { return check_step_args(h, fn, kBadSlotArgs, wav_in_host && state_dev && wav_out_host && (identity || slots_dev), n, capacity, T, in_stride, out_stride); },
        [&] {
            const size_t row = (size_t)T * h->d.HOP;
            const void* in = nullptr;
            const void* out = nullptr;
            int rc = pinned_view<float>(wav_in_host, (size_t)(n - 1) * in_stride + row, fn, "wav_in", &in);
            if (rc == FE_OK) rc = pinned_view<float>(wav_out_host, (size_t)(n - 1) * out_stride + row, fn, "wav_out", &out);
            if (rc == FE_OK && identity) rc = ensure_ident_slots(h, n);
            if (rc != FE_OK) return rc;
            fe::StreamFrameArgs own{};
            own.capacity = capacity; own.slots = identity ? h->ident_slots_dev : slots_dev;
            return launch_fe_step(h, fn, fe::STEP_SLOTS_PINNED, own, static_cast<const float*>(in), n > 1 ? in_stride : row, state_dev,
                                  const_cast<float*>(static_cast<const float*>(out)), n > 1 ? out_stride : row, n, T, stream);
        });
}

int fe_step_pinned(fe_handle* h, const float* wav_in_host, size_t in_stride, float* state_dev, float* wav_out_host, size_t out_stride,
                   int B, int T, void* stream) {
    return step_pinned(h, "fe_step_pinned", wav_in_host, in_stride, state_dev, B, nullptr, true, wav_out_host, out_stride, B, T, stream);
}

int fe_step_slots_pinned(fe_handle* h, const float* wav_in_host, size_t in_stride, float* state_dev, int capacity, const int* slots_dev,
                         float* wav_out_host, size_t out_stride, int n, int T, void* stream) {
    return step_pinned(h, "fe_step_slots_pinned", wav_in_host, in_stride, state_dev, capacity, slots_dev, false, wav_out_host, out_stride, n, T, stream);
}

// fe_step_streams / fe_step_streams_pinned: the launch fe_step_slots(n, T_max) makes, with the STRM instantiations - per-stream hop counts and audio
// offsets from desc_dev, float32 or int16 audio.  One set of kernels serves device and page-locked host audio: pinned only decides whether the two
// ranges are looked up (pinned_view) and how the kernel is named.  The descriptors' contents are the kernel's to check (fe_kernels.hip.h::stream_view).
static_assert(sizeof(fe_stream_desc) == 24 && sizeof(fe::StreamDesc) == 24 && offsetof(fe_stream_desc, slot) == offsetof(fe::StreamDesc, slot) &&
              offsetof(fe_stream_desc, hops) == offsetof(fe::StreamDesc, hops) && offsetof(fe_stream_desc, in_offset) == offsetof(fe::StreamDesc, in_offset) &&
              offsetof(fe_stream_desc, out_offset) == offsetof(fe::StreamDesc, out_offset), "fe_stream_desc is the kernels' StreamDesc");
static_assert(sizeof(fe_stream_levels) == 16 && sizeof(fe::StreamLevels) == 16 && offsetof(fe_stream_levels, in_peak) == offsetof(fe::StreamLevels, in_peak) &&
              offsetof(fe_stream_levels, out_sumsq) == offsetof(fe::StreamLevels, out_sumsq) && offsetof(fe_stream_levels, out_peak) == offsetof(fe::StreamLevels, out_peak),
              "fe_stream_levels is the kernels' StreamLevels");
// min_gain / levels (fe_step_streams_ctl[_pinned]; null from fe_step_streams[_pinned]): the two slot-indexed tables, `bytes` each from p.  Device memory
// is handed to the kernel as it comes, page-locked host memory as its device view; memory the device cannot reach (pageable host memory would
// make the kernel take a page fault) is refused here, before any launch.
static int table_view(const void* p, size_t bytes, const char* fn, const char* what, const void** dev) {
    *dev = p;
    if (!p) return FE_OK;
    const char* ends[2] = {static_cast<const char*>(p), static_cast<const char*>(p) + (bytes - 1)};
    const char* dv[2] = {nullptr, nullptr};
    for (int i = 0; i < 2; ++i) {
        hipPointerAttribute_t at{};
        bool ok = hipPointerGetAttributes(&at, ends[i]) == hipSuccess && (at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeHost || at.type == hipMemoryTypeManaged);
        void* dp = const_cast<char*>(ends[i]);
        if (ok && at.type == hipMemoryTypeHost) ok = hipHostGetDevicePointer(&dp, const_cast<char*>(ends[i]), 0) == hipSuccess && dp != nullptr;
        (void)hipGetLastError();        // (a refused lookup must not surface as the error of a later launch)
        if (!ok)
            return fail(FE_ERR_INVALID_ARG, "%s: %s is neither device memory nor page-locked host memory mapped for this device (%s byte of the table)", fn, what,
                        i ? "last" : "first");
        dv[i] = static_cast<const char*>(dp);
    }
    if (dv[1] - dv[0] != ends[1] - ends[0]) return fail(FE_ERR_INVALID_ARG, "%s: %s spans more than one allocation", fn, what);
    *dev = dv[0];
    return FE_OK;
}
// chunk (fe_step_streams_chunk[_pinned]): the same call with each stream's hops on the time pipeline where streams_chunk_pipe_width says so and
// the runtime accepts the cooperative launch (launch_streams_chunk, below fe_step_chunk); otherwise - and always after the same checks - the
// launch of the packet step itself.
static int streams_chunk_pipe_width(const fe_handle* h, int n, int T_max);
static int launch_streams_chunk(fe_handle* h, const fe::StreamFrameArgs& own, const float* wav_in, float* state, float* wav_out, int n, int T_max, int P,
                                float* work_dev, void* stream, bool* refused);
// the packet steps' own argument checks (fe_step_streams*, fe_step_pool_streams*), under the entry point's name
static int check_streams_args(const char* fn, const void* wav_in, size_t in_count, const float* state_dev, int capacity, const fe_stream_desc* desc_dev,
                              const void* wav_out, size_t out_count, int n, int T_max, int format, const fe_stream_levels* levels) {
    if (!wav_in || !state_dev || !desc_dev || !wav_out || n <= 0 || T_max <= 0 || capacity < n || in_count == 0 || out_count == 0)
        return fail(FE_ERR_INVALID_ARG, "%s: bad argument (need non-null pointers to at least one element, 1 <= n <= capacity, T_max >= 1)", fn);
    if (format != FE_AUDIO_F32 && format != FE_AUDIO_S16)
        return fail(FE_ERR_INVALID_ARG, "%s: format %d is neither FE_AUDIO_F32 (0) nor FE_AUDIO_S16 (1)", fn, format);
    if (reinterpret_cast<size_t>(levels) & 15)
        return fail(FE_ERR_INVALID_ARG, "%s: levels is not 16-byte aligned (the kernel writes each row as one 16-byte store)", fn);
    return FE_OK;
}
// ... and what their kernels get as wav_in / wav_out: the whole of both buffers, [wav, wav + count) in elements of the format - what the kernel's own
// bounds check confines every access to.  pinned: the device views of the two ranges, both ends of each looked up.
static int streams_audio(const char* fn, bool pinned, int format, const void* wav_in, size_t in_count, const void* wav_out, size_t out_count, const void** in,
                         const void** out) {
    *in = wav_in;
    *out = wav_out;
    if (!pinned) return FE_OK;
    const auto view = format == FE_AUDIO_S16 ? &pinned_view<short> : &pinned_view<float>;
    const int rc = view(wav_in, in_count, fn, "wav_in", in);
    return rc != FE_OK ? rc : view(wav_out, out_count, fn, "wav_out", out);
}
static int step_streams(fe_handle* h, const char* fn, bool pinned, const void* wav_in, size_t in_count, float* state_dev, int capacity,
                        const fe_stream_desc* desc_dev, void* wav_out, size_t out_count, int n, int T_max, int format, void* stream,
                        const float* min_gain = nullptr, fe_stream_levels* levels = nullptr, const int* bank = nullptr, bool chunk = false,
                        float* work_dev = nullptr) {
    return slotted_step(h, fn, true,
        [&]() -> int { return check_streams_args(fn, wav_in, in_count, state_dev, capacity, desc_dev, wav_out, out_count, n, T_max, format, levels); },
        [&]() -> int {
            const void* in = nullptr;
            const void* out = nullptr;
            int rc = streams_audio(fn, pinned, format, wav_in, in_count, wav_out, out_count, &in, &out);
            if (rc != FE_OK) return rc;
            fe::StreamFrameArgs own{};
            own.capacity = capacity;
            own.desc = reinterpret_cast<const fe::StreamDesc*>(desc_dev);
            own.in_count = in_count; own.out_count = out_count;
            own.format = format;
            own.pinned = pinned ? 1 : 0;
            const void* gains = nullptr;
            const void* rows = nullptr;
            const void* banks = nullptr;
            rc = table_view(min_gain, (size_t)capacity * sizeof(float), fn, "min_gain", &gains);
            if (rc == FE_OK) rc = table_view(levels, (size_t)capacity * sizeof(fe_stream_levels), fn, "levels", &rows);
            if (rc == FE_OK) rc = table_view(bank, (size_t)capacity * sizeof(int), fn, "bank", &banks);
            if (rc != FE_OK) return rc;
            own.min_gain = static_cast<const float*>(gains);
            own.levels = static_cast<fe::StreamLevels*>(const_cast<void*>(rows));
            if (bank) {       // (the table's contents are the kernel's to read: every bank it may name must hold a checkpoint)
                for (int k = 0; k < h->n_banks; ++k)
                    if (!h->bank_loaded[(size_t)k])
                        return fail(FE_ERR_NO_WEIGHTS, "%s: bank %d of the handle's %d has no weights (fe_load_weights_bank)", fn, k, h->n_banks);
                own.bank = static_cast<const int*>(banks);
                own.n_banks = h->n_banks;
                own.bank_stride = h->bank_stride;
            }
            if (const int P = chunk ? streams_chunk_pipe_width(h, n, T_max) : 0) {
                if (!work_dev) return fail(FE_ERR_INVALID_ARG, "%s: null work buffer (fe_step_streams_chunk_work_floats(h, %d, %d) floats)", fn, n, T_max);
                bool refused = false;
                rc = launch_streams_chunk(h, own, static_cast<const float*>(in), state_dev, const_cast<float*>(static_cast<const float*>(out)), n, T_max, P,
                                          work_dev, stream, &refused);
                if (!refused) return rc;
                // the runtime refused co-residency (GPU shared with other work): the packet step's own launch
            }
            return launch_fe_step(h, fn, fe::STEP_STREAMS, own, static_cast<const float*>(in), 0, state_dev, const_cast<float*>(static_cast<const float*>(out)), 0,
                                  n, T_max, stream);       // (the audio is typed by a.format in the kernel)
        });
}

int fe_step_streams(fe_handle* h, const void* wav_in_dev, size_t in_count, float* state_dev, int capacity, const fe_stream_desc* desc_dev,
                    void* wav_out_dev, size_t out_count, int n, int T_max, int format, void* stream) {
    return step_streams(h, "fe_step_streams", false, wav_in_dev, in_count, state_dev, capacity, desc_dev, wav_out_dev, out_count, n, T_max, format, stream);
}

// fe_step_pool_streams / fe_step_pool_streams_pinned: the packet step for every family with a streaming state - to fe_step_streams[_pinned] what
// fe_step_pool is to fe_step_slots.  FastEnhancer's handles take step_streams' path as it stands, under this entry point's name (the noncausal
// model its refusal, which is fe_step's); a baseline family runs the launches fe_step_pool(n, T = T_max) picks, in their packet instantiations,
// with step_streams' checks in step_streams' order.  Nothing is allocated.
// min_gain / levels (fe_step_pool_streams_ctl[_pinned]; null from fe_step_pool_streams[_pinned]): the two slot-indexed tables, looked up as
// step_streams looks them up (table_view) and handed to the same launches - the packet instantiations apply them behind null tests.
// chunk (fe_step_pool_streams_chunk[_pinned]): the same call with each stream's hops on the family's time pipeline where
// pool_streams_chunk_pipe_width says so and the runtime accepts the cooperative launch (launch_pool_streams_chunk, below fe_step_backlog);
// otherwise - and always after the same checks - the launch of the packet step itself.  FastEnhancer: fe_step_streams_chunk without a bank table.
static int pool_streams_chunk_pipe_width(const fe_handle* h, int n, int T_max, const float* work_dev);
static int launch_pool_streams_chunk(fe_handle* h, const BaselineStepOwn& own, const float* wav_in, float* state, float* wav_out, int n, int T_max, int P,
                                     float* work_dev, void* stream, bool* refused);
static int step_pool_streams(fe_handle* h, const char* fn, bool pinned, const void* wav_in, size_t in_count, float* state_dev, int capacity,
                             const fe_stream_desc* desc_dev, void* wav_out, size_t out_count, int n, int T_max, int format, void* stream,
                             const float* min_gain = nullptr, fe_stream_levels* levels = nullptr, bool chunk = false, float* work_dev = nullptr) {
    if (!h) return fail(FE_ERR_INVALID_ARG, "null handle");
    if (h->cfg.arch == FE_ARCH_FASTENHANCER)
        return step_streams(h, fn, pinned, wav_in, in_count, state_dev, capacity, desc_dev, wav_out, out_count, n, T_max, format, stream, min_gain, levels,
                            nullptr, chunk, work_dev);
    int rc = check_streams_args(fn, wav_in, in_count, state_dev, capacity, desc_dev, wav_out, out_count, n, T_max, format, levels);
    if (rc != FE_OK) return rc;
    const int P = chunk ? pool_streams_chunk_pipe_width(h, n, T_max, work_dev) : 0;
    // (a family that pipelines on request has P = 0 without a buffer: the packet step itself, no error)
    if (P && !work_dev) return fail(FE_ERR_INVALID_ARG, "%s: null work buffer (fe_step_pool_streams_chunk_work_floats(h, %d, %d) floats)", fn, n, T_max);
    rc = check_ready(h);
    if (rc != FE_OK) return rc;
    KernelLogScope klog_(h);
    const void* in = nullptr;
    const void* out = nullptr;
    rc = streams_audio(fn, pinned, format, wav_in, in_count, wav_out, out_count, &in, &out);
    const void* gains = nullptr;
    const void* rows = nullptr;
    if (rc == FE_OK) rc = table_view(min_gain, (size_t)capacity * sizeof(float), fn, "min_gain", &gains);
    if (rc == FE_OK) rc = table_view(levels, (size_t)capacity * sizeof(fe_stream_levels), fn, "levels", &rows);
    if (rc != FE_OK) return rc;
    BaselineStepOwn own;
    own.capacity = capacity;
    own.io = fe::StreamIoArgs{reinterpret_cast<const fe::StreamDesc*>(desc_dev), in_count, out_count, format, pinned ? 1 : 0,
                              static_cast<const float*>(gains), static_cast<fe::StreamLevels*>(const_cast<void*>(rows))};
    // (the audio is typed by the format in the kernel)
    if (P) {
        bool refused = false;
        rc = launch_pool_streams_chunk(h, own, static_cast<const float*>(in), state_dev, const_cast<float*>(static_cast<const float*>(out)), n, T_max, P, work_dev,
                                       stream, &refused);
        if (!refused) return rc;
        // the runtime refused co-residency (GPU shared with other work): the packet step's own launch
    }
    return launch_baseline_step(h, fe::STEP_STREAMS, own, static_cast<const float*>(in), 0, state_dev, const_cast<float*>(static_cast<const float*>(out)), 0, n,
                                T_max, stream);
}

int fe_step_pool_streams(fe_handle* h, const void* wav_in_dev, size_t in_count, float* state_dev, int capacity, const fe_stream_desc* desc_dev,
                         void* wav_out_dev, size_t out_count, int n, int T_max, int format, void* stream) {
    return step_pool_streams(h, "fe_step_pool_streams", false, wav_in_dev, in_count, state_dev, capacity, desc_dev, wav_out_dev, out_count, n, T_max, format, stream);
}

int fe_step_pool_streams_pinned(fe_handle* h, const void* wav_in_host, size_t in_count, float* state_dev, int capacity, const fe_stream_desc* desc_dev,
                                void* wav_out_host, size_t out_count, int n, int T_max, int format, void* stream) {
    return step_pool_streams(h, "fe_step_pool_streams_pinned", true, wav_in_host, in_count, state_dev, capacity, desc_dev, wav_out_host, out_count, n, T_max, format,
                             stream);
}

int fe_step_pool_streams_ctl(fe_handle* h, const void* wav_in_dev, size_t in_count, float* state_dev, int capacity, const fe_stream_desc* desc_dev,
                             void* wav_out_dev, size_t out_count, int n, int T_max, int format, const float* min_gain, fe_stream_levels* levels, void* stream) {
    return step_pool_streams(h, "fe_step_pool_streams_ctl", false, wav_in_dev, in_count, state_dev, capacity, desc_dev, wav_out_dev, out_count, n, T_max, format,
                             stream, min_gain, levels);
}

int fe_step_pool_streams_ctl_pinned(fe_handle* h, const void* wav_in_host, size_t in_count, float* state_dev, int capacity, const fe_stream_desc* desc_dev,
                                    void* wav_out_host, size_t out_count, int n, int T_max, int format, const float* min_gain, fe_stream_levels* levels,
                                    void* stream) {
    return step_pool_streams(h, "fe_step_pool_streams_ctl_pinned", true, wav_in_host, in_count, state_dev, capacity, desc_dev, wav_out_host, out_count, n, T_max,
                             format, stream, min_gain, levels);
}

int fe_step_streams_pinned(fe_handle* h, const void* wav_in_host, size_t in_count, float* state_dev, int capacity, const fe_stream_desc* desc_dev,
                           void* wav_out_host, size_t out_count, int n, int T_max, int format, void* stream) {
    return step_streams(h, "fe_step_streams_pinned", true, wav_in_host, in_count, state_dev, capacity, desc_dev, wav_out_host, out_count, n, T_max, format, stream);
}

int fe_step_streams_ctl(fe_handle* h, const void* wav_in_dev, size_t in_count, float* state_dev, int capacity, const fe_stream_desc* desc_dev,
                        void* wav_out_dev, size_t out_count, int n, int T_max, int format, const float* min_gain, fe_stream_levels* levels, void* stream) {
    return step_streams(h, "fe_step_streams_ctl", false, wav_in_dev, in_count, state_dev, capacity, desc_dev, wav_out_dev, out_count, n, T_max, format, stream,
                        min_gain, levels);
}

int fe_step_streams_ctl_pinned(fe_handle* h, const void* wav_in_host, size_t in_count, float* state_dev, int capacity, const fe_stream_desc* desc_dev,
                               void* wav_out_host, size_t out_count, int n, int T_max, int format, const float* min_gain, fe_stream_levels* levels,
                               void* stream) {
    return step_streams(h, "fe_step_streams_ctl_pinned", true, wav_in_host, in_count, state_dev, capacity, desc_dev, wav_out_host, out_count, n, T_max, format,
                        stream, min_gain, levels);
}

// bank == NULL: the launch fe_step_streams_ctl[_pinned] makes (one code path: step_streams)
int fe_step_streams_banked(fe_handle* h, const void* wav_in_dev, size_t in_count, float* state_dev, int capacity, const fe_stream_desc* desc_dev,
                           void* wav_out_dev, size_t out_count, int n, int T_max, int format, const float* min_gain, fe_stream_levels* levels,
                           const int* bank, void* stream) {
    return step_streams(h, "fe_step_streams_banked", false, wav_in_dev, in_count, state_dev, capacity, desc_dev, wav_out_dev,
                        out_count, n, T_max, format, stream, min_gain, levels, bank);
}

int fe_step_streams_banked_pinned(fe_handle* h, const void* wav_in_host, size_t in_count, float* state_dev, int capacity, const fe_stream_desc* desc_dev,
                                  void* wav_out_host, size_t out_count, int n, int T_max, int format, const float* min_gain, fe_stream_levels* levels,
                                  const int* bank, void* stream) {
    return step_streams(h, "fe_step_streams_banked_pinned", true, wav_in_host, in_count, state_dev, capacity, desc_dev,
                        wav_out_host, out_count, n, T_max, format, stream, min_gain, levels, bank);
}

// The streaming state of `capacity` streams as a list of regions [rows][capacity][len], in the order of the layout (include/fastenhancer_hip.h):
// every family's state is such a list, so a stream's share of it - `len` floats in every row of every region - is what fe_state_reset_slots
// zeroes and what the state records of fe_state_export_slots / fe_state_import_slots hold.  Returns the number of regions.
static int state_regions(const fe_handle* h, size_t capacity, StateRegion* r) {
    const Dims& d = h->d;
    const StateLayout L = state_layout(h, capacity);
    const int ovl = d.NFFT - d.HOP;
    int nr = 0;
    r[nr++] = {0, 1, ovl};                                              // cache_stft [cap][N-H]
    r[nr++] = {L.cache_istft, 1, ovl};                                  // cache_istft [cap][N-H]
    if (visit_baseline(h->cfg.arch, [&](auto F) { nr += F.regions(h, capacity, L.h, r + nr); })) return nr;
    if (d.TA) {
        const int ring = d.F2 * d.C2 * d.TA;                              // K and V rings per block: [2 KB][cap][F2 * C2 * L], then the heads [cap]
        r[nr++] = {L.h, 2 * d.KB, ring};
        r[nr++] = {L.h + capacity * (size_t)(2 * d.KB) * ring, 1, 1};
    } else {
        r[nr++] = {L.h, d.KB, d.F2 * d.C2};                             // GRU states [KB][cap][F2 * C2]
    }
    if (d.KT > 1) r[nr++] = {L.tk, 2 * d.NL, (int)(tk_floats(h) / (2 * d.NL))};   // conv caches [2 NL][cap][KT-1][F1][C1]
    return nr;
}

// fe_state_reset_slots: what fe_state_init writes (zeros) for the named slots: one workgroup per named slot zeroes its len floats in every
// row of every region.
using ResetRegion = StateRegion;
struct ResetArgs {
    float* state;
    const int* slots;
    int capacity, n_regions;
    ResetRegion r[5];
};

__global__ void __launch_bounds__(256) state_reset_slots_kernel(ResetArgs a) {
    const int s = a.slots[blockIdx.x];
    if (s < 0 || s >= a.capacity) return;         // (out of range: nothing is written)
    for (int j = 0; j < a.n_regions; ++j) {
        const ResetRegion g = a.r[j];
        for (int row = 0; row < g.rows; ++row) {
            float* p = a.state + g.off + ((size_t)row * a.capacity + s) * g.len;
            for (int i = (int)threadIdx.x; i < g.len; i += (int)blockDim.x) p[i] = 0.0f;
        }
    }
}

int fe_state_reset_slots(fe_handle* h, float* state_dev, int capacity, const int* slots_dev, int n, void* stream) {
    if (!h) return fail(FE_ERR_INVALID_ARG, "null handle");
    int rc = check_slots_family(h, "fe_state_reset_slots");
    if (rc != FE_OK) return rc;
    if (!state_dev || !slots_dev || n <= 0 || capacity < n) return fail(FE_ERR_INVALID_ARG, "bad argument (need non-null pointers, 1 <= n <= capacity)");
    ResetArgs a{};
    a.state = state_dev;
    a.slots = slots_dev;
    a.capacity = capacity;
    StateRegion r[kMaxStateRegions];
    a.n_regions = state_regions(h, (size_t)capacity, r);          // (the FastEnhancer family: at most five)
    std::copy(r, r + a.n_regions, a.r);
    hipLaunchKernelGGL(state_reset_slots_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, a);
    return launch_rc(hipGetLastError());
}

// fe_state_export_slots / fe_state_import_slots: a stream's state record is the state of a capacity-1 batch, so the record side of a region
// is the same list at capacity 1 - the regions back to back, [rows][len] each - and moving a stream is a copy of its `len` floats of every row
// between the two lists.  One launch: grid (stream of the call, chunk of the record), so the workgroups follow the bytes, not the streams.
// A thread moves one 16-byte granule of the RECORD side at a time (consecutive lanes: consecutive granules, so both sides are read and written
// in runs of whole cache lines wherever a row is long enough); the granule grid is laid on the record's address, not its index, so that side is
// always aligned.  A granule that lies in one row and whose state address is 16-byte aligned too goes as one 16-byte load and store; any other
// one - row ends, the one-float `head`, regions whose two sides differ in alignment, the ragged ends of a record - float by float.
struct RecordRegion {
    size_t off;          // floats from the start of the state (at the call's capacity)
    int rec;             // floats from the start of a record (the same region at capacity 1)
    int rows, len;
};
struct RecordArgs {
    float* state;
    float* records;
    const int* slots;
    int capacity, n_regions;
    int rec_floats;      // floats per record
    int granules;        // granules per workgroup
    int to_state;        // 0: export (state -> records), 1: import
    RecordRegion r[kMaxStateRegions];
};
constexpr int kRecordGranules = 1024;      // 16 KB of a record per workgroup, four granules per thread

// where float e of a stream's record lives in the state (slot s): nullptr if e is outside the record
__device__ inline float* record_state_addr(const RecordArgs& a, int s, int e, int* left_in_row) {
    for (int j = 0; j < a.n_regions; ++j) {
        const RecordRegion g = a.r[j];
        const int k = e - g.rec;
        if (k < 0 || k >= g.rows * g.len) continue;
        const int row = k / g.len, i = k - row * g.len;
        *left_in_row = g.len - i;
        return a.state + g.off + ((size_t)row * a.capacity + s) * g.len + i;
    }
    return nullptr;
}

__global__ void __launch_bounds__(256) state_records_kernel(RecordArgs a) {
    const int s = a.slots[blockIdx.x];
    const bool live = s >= 0 && s < a.capacity;
    if (a.to_state && !live) return;                       // import of a slot out of range: nothing is written anywhere
    float* const rec = a.records + (size_t)blockIdx.x * a.rec_floats;
    const int shift = (int)((reinterpret_cast<size_t>(rec) >> 2) & 3);      // floats from the 16-byte boundary below rec
    const int g0 = (int)blockIdx.y * a.granules;
    for (int g = g0 + (int)threadIdx.x; g < g0 + a.granules; g += (int)blockDim.x) {
        const int e0 = 4 * g - shift;
        const int lo = e0 < 0 ? 0 : e0, hi = e0 + 4 < a.rec_floats ? e0 + 4 : a.rec_floats;
        if (lo >= hi) continue;
        const bool whole = hi - lo == 4;
        if (!live) {                                       // export of a slot out of range: the record of a fresh fe_state_init
            if (whole) *reinterpret_cast<float4*>(rec + lo) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            else for (int e = lo; e < hi; ++e) rec[e] = 0.0f;
            continue;
        }
        int left = 0;
        float* st = record_state_addr(a, s, lo, &left);
        if (whole && st && left >= 4 && (reinterpret_cast<size_t>(st) & 15) == 0) {
            if (a.to_state) *reinterpret_cast<float4*>(st) = *reinterpret_cast<const float4*>(rec + lo);
            else *reinterpret_cast<float4*>(rec + lo) = *reinterpret_cast<const float4*>(st);
            continue;
        }
        for (int e = lo; e < hi; ++e) {
            if (left <= 0) st = record_state_addr(a, s, e, &left);
            if (!st) break;
            if (a.to_state) *st = rec[e]; else rec[e] = *st;
            ++st; --left;
        }
    }
}

// `count` floats from p as the kernel may address them: device memory of the current device as it is, or the device view of page-locked host
// memory mapped for it (pinned_view).  Both ends of the range are looked up; pageable memory, or memory of another device, is refused.
static int records_view(const float* p, size_t count, const char* fn, const float** dev) {
    int cur = -1;
    FE_HIP_CHECK(hipGetDevice(&cur));
    const float* ends[2] = {p, p + (count - 1)};
    bool device = true;
    for (int i = 0; i < 2 && device; ++i) {
        hipPointerAttribute_t at{};
        device = hipPointerGetAttributes(&at, ends[i]) == hipSuccess && at.type == hipMemoryTypeDevice && at.device == cur;
        (void)hipGetLastError();
    }
    if (device) { *dev = p; return FE_OK; }
    const void* v = nullptr;
    const int rc = pinned_view<float>(p, count, fn, "records", &v);
    if (rc != FE_OK)
        return fail(FE_ERR_INVALID_ARG, "%s: records is neither memory of the current device nor page-locked host memory mapped for it, from its first to its "
                    "last float: pin a host buffer as one piece (torch: pin_memory(); C: hipHostMalloc / hipHostRegister)", fn);
    *dev = static_cast<const float*>(v);
    return FE_OK;
}

static int state_records(fe_handle* h, const char* fn, bool to_state, float* state_dev, int capacity, const int* slots_dev, float* records, int n, void* stream) {
    if (!h) return fail(FE_ERR_INVALID_ARG, "null handle");
    if (h->cfg.arch == FE_ARCH_FASTENHANCER && h->d.BD) return fail(FE_ERR_UNSUPPORTED_CONFIG, "%s", kNoncausalNoStep);
    if (!state_dev || !slots_dev || !records || n <= 0 || capacity < n)
        return fail(FE_ERR_INVALID_ARG, "%s: bad argument (need non-null pointers, 1 <= n <= capacity)", fn);
    RecordArgs a{};
    StateRegion at_cap[kMaxStateRegions], at_one[kMaxStateRegions];
    a.n_regions = state_regions(h, (size_t)capacity, at_cap);
    state_regions(h, 1, at_one);
    const size_t rec = fe_state_floats(h, 1);
    size_t covered = 0;
    for (int j = 0; j < a.n_regions; ++j) {
        if (at_one[j].off != covered) break;               // (the regions of one stream lie back to back: that is what makes them a record)
        a.r[j] = {at_cap[j].off, (int)at_one[j].off, at_cap[j].rows, at_cap[j].len};
        covered += (size_t)at_one[j].rows * at_one[j].len;
    }
    if (covered != rec || rec >= (size_t)1 << 30) return fail(FE_ERR_UNSUPPORTED_CONFIG, "%s: the state's regions do not add up to fe_state_floats(h, 1)", fn);
    const float* view = nullptr;
    const int rc = records_view(records, (size_t)n * rec, fn, &view);
    if (rc != FE_OK) return rc;
    a.state = state_dev;
    a.records = const_cast<float*>(view);
    a.slots = slots_dev;
    a.capacity = capacity;
    a.rec_floats = (int)rec;
    a.to_state = to_state ? 1 : 0;
    // (+ 1: a record that does not start on a 16-byte boundary touches one granule more)
    const size_t granules = (rec + 3) / 4 + 1;
    // few streams: smaller chunks, so that a handful of large records still spreads over the device (at least one round of 256 threads each)
    a.granules = kRecordGranules;
    while (a.granules > 256 && (size_t)n * ((granules + a.granules - 1) / a.granules) < (size_t)2 * h->max_wgs) a.granules /= 2;
    while ((granules + a.granules - 1) / a.granules > 65535) a.granules *= 2;          // (the grid's second dimension)
    const size_t chunks = (granules + a.granules - 1) / a.granules;
    return launch_rc(fe::launch<state_records_kernel>(to_state ? "state_records_kernel<import>" : "state_records_kernel<export>",
                                                      dim3((unsigned)n, (unsigned)chunks), dim3(256), 0, (hipStream_t)stream, a));
}

int fe_state_export_slots(fe_handle* h, const float* state_dev, int capacity, const int* slots_dev, float* records, int n, void* stream) {
    return state_records(h, "fe_state_export_slots", false, const_cast<float*>(state_dev), capacity, slots_dev, records, n, stream);
}

int fe_state_import_slots(fe_handle* h, float* state_dev, int capacity, const int* slots_dev, const float* records, int n, void* stream) {
    return state_records(h, "fe_state_import_slots", true, state_dev, capacity, slots_dev, const_cast<float*>(records), n, stream);
}

int fe_step_host(fe_handle* h, const float* wav_in_host, size_t in_stride, float* state_dev, float* wav_out_host, size_t out_stride,
                 int B, int T, int n_calls, float* work_dev, void* stream) {
    int rc = check_ready(h);
    if (rc != FE_OK) return rc;
    if (!wav_in_host || !wav_out_host || !state_dev || !work_dev || B <= 0 || T <= 0 || n_calls <= 0) return fail(FE_ERR_INVALID_ARG, "bad argument");
    hipStream_t st = (hipStream_t)stream;
    for (hipStream_t& s : h->host_streams)
        if (!s) FE_HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    for (hipEvent_t& e : h->host_events)
        if (!e) FE_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    hipStream_t s_in = h->host_streams[0], s_out = h->host_streams[1];
    // events: [0] start, [1 + buf] block copied in, [3 + buf] block computed, [5 + buf] block copied out
    hipEvent_t* ev = h->host_events;
    const size_t row = (size_t)T * h->d.HOP, blk = (size_t)B * row;
    float* xd[2] = {work_dev, work_dev + blk};
    float* yd[2] = {work_dev + 2 * blk, work_dev + 3 * blk};
    FE_HIP_CHECK(hipEventRecord(ev[0], st));
    FE_HIP_CHECK(hipStreamWaitEvent(s_in, ev[0], 0));
    FE_HIP_CHECK(hipStreamWaitEvent(s_out, ev[0], 0));
    for (int c = 0; c < n_calls; ++c) {
        const int buf = c & 1;
        // copy-in of block c: its staging buffer was last read by the kernel of block c - 2
        if (c >= 2) FE_HIP_CHECK(hipStreamWaitEvent(s_in, ev[3 + buf], 0));
        FE_HIP_CHECK(hipMemcpy2DAsync(xd[buf], row * sizeof(float), wav_in_host + (size_t)c * row, in_stride * sizeof(float), row * sizeof(float), (size_t)B,
                                      hipMemcpyHostToDevice, s_in));
        FE_HIP_CHECK(hipEventRecord(ev[1 + buf], s_in));
        // kernel of block c: input landed, and the output staging buffer has been copied out (block c - 2)
        FE_HIP_CHECK(hipStreamWaitEvent(st, ev[1 + buf], 0));
        if (c >= 2) FE_HIP_CHECK(hipStreamWaitEvent(st, ev[5 + buf], 0));
        rc = run_step(h, xd[buf], row, state_dev, yd[buf], row, B, T, nullptr, nullptr, stream);
        if (rc != FE_OK) return rc;
        FE_HIP_CHECK(hipEventRecord(ev[3 + buf], st));
        // copy-out of block c
        FE_HIP_CHECK(hipStreamWaitEvent(s_out, ev[3 + buf], 0));
        FE_HIP_CHECK(hipMemcpy2DAsync(wav_out_host + (size_t)c * row, out_stride * sizeof(float), yd[buf], row * sizeof(float), row * sizeof(float), (size_t)B,
                                      hipMemcpyDeviceToHost, s_out));
        FE_HIP_CHECK(hipEventRecord(ev[5 + buf], s_out));
    }
    for (int buf = 0; buf < (n_calls < 2 ? n_calls : 2); ++buf) FE_HIP_CHECK(hipStreamWaitEvent(st, ev[5 + buf], 0));
    return FE_OK;
}

int fe_debug_step(fe_handle* h, const float* wav_in_dev, size_t in_stride, float* state_dev, float* wav_out_dev,
                  size_t out_stride, int B, float* dbg_dev, void* stream) {
    if (!dbg_dev) return fail(FE_ERR_INVALID_ARG, "null dbg buffer");
    return run_step(h, wav_in_dev, in_stride, state_dev, wav_out_dev, out_stride, B, 1, dbg_dev, nullptr, stream);
}

int fe_profile_step(fe_handle* h, const float* wav_in_dev, size_t in_stride, float* state_dev, float* wav_out_dev,
                    size_t out_stride, int B, int T, unsigned long long* clk_dev, void* stream) {
    if (!clk_dev) return fail(FE_ERR_INVALID_ARG, "null clock buffer");
    return run_step(h, wav_in_dev, in_stride, state_dev, wav_out_dev, out_stride, B, T, nullptr, clk_dev, stream);
}

// workgroups per stream of a time-pipelined launch (0: one workgroup walks the frames of a stream).  The ring variants (time_kernel: its
// convs' inputs, dptransformer: K / V, handed from frame to frame through rings) pipeline wherever their caller supplies the rings, and
// every caller does: fe_offline and fe_step_chunk in their work buffers, fe_spec_step in the handle's (r4v); the packet chunk never asks.
static int pipe_width(const fe_handle* h, int B, int T) {
    if (!h->impl || h->pipe_frames == 0 || h->pipe_frames == 1 || T < 4 || 2 * B > h->max_wgs) return 0;
    // automatic width: a hand-off (counter round trip + state fetch + the h half of the GRU + gates + publish) takes
    // ~2.6 us whatever the model; a frame takes ~4 us per MFLOP/frame at the measured kernel efficiency: that many frames
    // are worth having in flight (measured optimum: T 8-12, B 16, 48 kHz B 24, L > 24), more only adds pollers
    int want = h->pipe_frames;
    if (want < 0) {
        want = (int)(fe_flops_per_frame(h) / 6.0e5) + 2;
        if (h->d.TA) want *= 2;     // (dptransformer: a frame spends half its time streaming its K / V window - measured 16 -> 32 in flight: 1.37 -> 0.73 ms)
        want = want < 8 ? 8 : (want > kMaxPipeFrames ? kMaxPipeFrames : want);
    }
    int p = h->max_wgs / B;
    p = p < want ? p : want;
    return p < T ? p : T;
}

// frame counters per stream of a time-pipelined launch (fe_kernels.hip.h: NFLAG)
static size_t pipe_counters(const fe_handle* h) { return (size_t)h->d.KB + (h->d.KT > 1 ? 2 * h->d.NL : 0); }

// floats of the rings a time-pipelined chunk with carried caches needs at width P: dptransformer - per (K / V cache, stream, pair) TA + P
// slots of a head's channels; time_kernel - per (conv, stream) KT - 1 + P slots of [F1][C1]; 0 for the other variants
static size_t pipe_ring_floats(const fe_handle* h, int B, int P) {
    const Dims& d = h->d;
    if (d.TA) return (size_t)2 * d.KB * B * d.F2 * d.C2 * (d.TA + P);
    if (d.KT > 1) return (size_t)2 * d.NL * B * (d.KT - 1 + P) * d.F1 * d.C1;
    return 0;
}

// FastEnhancer's pipeline region, the rings at the widest pipeline: the work buffer of fe_step_chunk and of fe_step_streams_chunk (whose
// models have no rings).  The size depends on the model, rows and T only - not on fe_set_time_pipeline nor on the device's CUs - so that
// it is monotone in both and a buffer sized once serves every setting.
static PipeLayout fe_pipe_layout(const fe_handle* h, int rows, int T) {
    return pipe_layout(h, rows, T, pipe_counters(h), pipe_ring_floats(h, rows, kMaxPipeFrames));
}

// FastEnhancer's fe_offline on the frame walk: the state is h (GRU states or K / V caches) | tk (the time_kernel conv caches), not rounded
static OfflineLayout fe_walk_layout(const fe_handle* h, int B, int T) {
    return offline_layout(h, B, T, (size_t)B * (h->d.hstate() + tk_floats(h)), pipe_counters(h), pipe_ring_floats(h, B, kMaxPipeFrames));
}

// The time-batched engine's work buffer, each region a multiple of 4 floats.  (`spare` held the GRU state carried between time chunks;
// nothing writes it any more - it stays in the total so that the sizes callers were given stay what they are.)
struct TbLayout { size_t xc, skip, x, gx, hs, frames, spare, total; };
static TbLayout tb_layout(const fe_handle* h, int B, int T) {
    const Dims& d = h->d;
    const size_t NF = (size_t)B * T, nd = d.BD ? 2 : 1;
    size_t cur = 0;
    auto region = [&](size_t floats) { const size_t at = cur; cur += round4(floats); return at; };
    return {region(NF * 2 * d.F0), region(NF * (d.NL + 1) * d.F1 * d.C1), region(NF * d.F2 * d.C2), region(nd * NF * d.F2 * 3 * d.C2),
            region(NF * d.F2 * nd * d.C2), region(NF * d.NFFT), region((size_t)d.KB * nd * B * d.F2 * d.C2), cur};      // (in this order)
}

// The time-pipelined launch of a chunk that starts from the caller's model caches and leaves the new ones - fe_spec_step and fe_step_chunk.
// a: the serial walk's launch (a.h / a.tk point into h_dev, the model caches of B streams in C ABI order) with the pipeline's fields set -
// a.pipe_p: pipe_width's answer; a.pipe_flags: pipe_counters() x B counters, zeroed here; ring: pipe_ring_floats(h, B, a.pipe_p) floats.
// The GRU states are read from and written to h_dev by the kernel itself.  dptransformer / time_kernel (r4v): the frames of a chunk in
// flight exchange their k / v (their convs' inputs) through rings of L + P slots; the caller's caches go in before the launch and the
// chunk's last L frames come back after it (ring_in_kernel / ring_out_kernel above).  *refused: the runtime refused the cooperative
// launch and nothing has been written that the serial walk of the caller's own block does not overwrite or ignore.
static int launch_pipe_carried(fe_handle* h, fe::StreamFrameArgs a, float* h_dev, int B, int T, float* ring, hipStream_t st, bool* refused) {
    const Dims& d = h->d;
    *refused = false;
    FE_HIP_CHECK(hipMemsetAsync(a.pipe_flags, 0, (size_t)B * pipe_counters(h) * sizeof(unsigned int), st));
    const bool rings = d.TA != 0 || d.KT > 1;
    const int L = d.TA ? d.TA : d.KT - 1, RS = L + a.pipe_p;
    const int PAIRS = d.TA ? d.F2 * 4 : 1, SZ = d.TA ? d.C2 / 4 : d.F1 * d.C1;
    const size_t rows = (size_t)(d.TA ? 2 * d.KB : 2 * d.NL) * B * PAIRS, nfl = rows * L * SZ;
    float* caches = d.TA ? h_dev : h_dev + (size_t)B * d.hstate();
    float* heads = d.TA ? h_dev + (size_t)B * (d.hstate() - 1) : nullptr;     // (the ring heads sit behind the K / V caches: fe_kernels.hip.h, ring_head0)
    const unsigned cgrid = (unsigned)((nfl + 255) / 256);
    if (rings) {
        hipLaunchKernelGGL(ring_in_kernel, dim3(cgrid), dim3(256), 0, st, caches, heads, ring, nfl, B, PAIRS, SZ, L, RS);
        if (d.TA) { a.h = ring; a.tatt_base = d.TA; }
        else { a.tk = ring; a.tk_base = d.KT - 1; }
    }
    hipError_t e = hipSuccess;
    h->impl->launch_pipe(a, st, &e);
    if ((*refused = coop_refused(e))) return FE_OK;
    if (rings) {
        hipLaunchKernelGGL(ring_out_kernel, dim3(cgrid), dim3(256), 0, st, ring, caches, heads, nfl, B, SZ, L, RS, T);
        e = hipGetLastError();
    }
    return launch_rc(e);
}

int fe_set_time_pipeline(fe_handle* h, int frames_in_flight) {
    if (!h) return fail(FE_ERR_INVALID_ARG, "bad argument");
    // The per-frame rings in work_dev (time_kernel inputs, dptransformer K / V, LiSenNet caches) are sized for at most kMaxPipeFrames
    // frames in flight (fe_offline_work_floats), and more never paid on any model: larger requests are clamped, not refused.
    h->pipe_frames = frames_in_flight > kMaxPipeFrames ? kMaxPipeFrames : frames_in_flight;
    return FE_OK;
}

static int tb_run(fe_handle* h, fe::tb::TbArgs a, float* work_dev, int B, int T, hipStream_t st);

// spec -> spec chunks on the time-batched engine: when asked for (FE_OFFLINE_TIME_BATCHED), or - AUTO - for long chunks of batches that
// the time pipeline cannot take (more than #CUs / 2 streams: each workgroup would walk its T frames alone) or that are simply large
static bool use_tb_spec(const fe_handle* h, int B, int T) {
    if (!h->impl || !h->impl->tb || h->d.BD || h->offline_engine == FE_OFFLINE_FRAME_WALK || T < 2) return false;
    if (h->offline_engine == FE_OFFLINE_TIME_BATCHED) return true;
    if (h->d.C2 >= 72) return false;
    // ("cannot take" = too many streams - NOT a caller's fe_set_time_pipeline(0 / 1), which asks for the serial walk and gets it)
    if (h->pipe_frames == 0 || h->pipe_frames == 1) return false;
    return T >= 16 && (2 * B > h->max_wgs || (long)B * T >= 2048);
}

int fe_spec_step(fe_handle* h, const float* spec_in_dev, float* h_dev, float* spec_out_dev, int B, int T, void* stream) {
    int rc = check_ready(h);
    if (rc != FE_OK) return rc;
    KernelLogScope klog_(h);
    if (!spec_in_dev || !h_dev || !spec_out_dev || B <= 0 || T <= 0) return fail(FE_ERR_INVALID_ARG, "bad argument");
    if (visit_baseline(h->cfg.arch, [&](auto F) {
            auto a = F.args(h, B, T);
            a.mode = fe::FE_MODE_SPEC;
            a.spec_in = spec_in_dev; a.spec_out = spec_out_dev; F.state(a) = h_dev;
            rc = F.launch_step(h, a, fe::STEP_PLAIN, stream);
        }))
        return rc;
    if (h->d.BD) return fail(FE_ERR_UNSUPPORTED_CONFIG, "the noncausal model has no spec -> spec step with caches (models/fastenhancer/noncausal/model.py has the offline Model only): use fe_offline");
    if (use_tb_spec(h, B, T)) {
        // the chunk as one encoder pass, per block a scan that starts from the caller's GRU state and leaves the new one + a tile pass,
        // one decoder pass (fe_spec_step has no work buffer argument: the handle keeps a grow-only one - a first / larger call allocates)
        const size_t need = tb_layout(h, B, T).total;
        if (need > h->tb_work_floats) {
            if (h->tb_work_dev) { FE_HIP_CHECK(hipFree(h->tb_work_dev)); h->tb_work_dev = nullptr; h->tb_work_floats = 0; }
            FE_HIP_CHECK(hipMalloc(&h->tb_work_dev, need * sizeof(float)));
            h->tb_work_floats = need;
        }
        fe::tb::TbArgs ta{};
        ta.wp = h->packed_dev;
        ta.spec_in = spec_in_dev; ta.spec_out = spec_out_dev;
        ta.hstate = h_dev; ta.h_init = 1;
        ta.mode = fe::FE_MODE_SPEC;
        ta.compression = h->cfg.input_compression;
        return tb_run(h, ta, h->tb_work_dev, B, T, (hipStream_t)stream);
    }
    rc = ensure_scratch(h, B);
    if (rc != FE_OK) return rc;
    fe::StreamFrameArgs a = base_args(h, B, T);
    a.spec_in = spec_in_dev;
    a.spec_out = spec_out_dev;
    a.h = h_dev;
    a.tk = h_dev + (size_t)B * h->d.hstate();
    hipError_t e = hipSuccess;
    a.mode = fe::FE_MODE_SPEC;
    if (const int P = pipe_width(h, B, T)) {
        hipStream_t st = (hipStream_t)stream;
        const size_t nflags = (size_t)h->max_wgs * pipe_counters(h);
        if (!h->pipe_flags_dev) FE_HIP_CHECK(hipMalloc(&h->pipe_flags_dev, nflags * sizeof(unsigned int)));
        // (the handle keeps the rings of the dptransformer / time_kernel variants: grow-only, a first / wider call allocates)
        const size_t need = pipe_ring_floats(h, B, P);
        if (need > h->spec_ring_floats) {
            if (h->spec_ring_dev) { FE_HIP_CHECK(hipFree(h->spec_ring_dev)); h->spec_ring_dev = nullptr; h->spec_ring_floats = 0; }
            FE_HIP_CHECK(hipMalloc(&h->spec_ring_dev, need * sizeof(float)));
            h->spec_ring_floats = need;
        }
        fe::StreamFrameArgs p = a;
        p.pipe_flags = h->pipe_flags_dev;
        p.pipe_p = P;
        bool refused = false;
        rc = launch_pipe_carried(h, p, h_dev, B, T, h->spec_ring_dev, st, &refused);
        if (!refused) return rc;
        // the runtime refused co-residency (GPU shared with other work): walk the frames serially
    }
    h->impl->launch_step(a, fe::STEP_PLAIN, h->max_wgs, (hipStream_t)stream, &e);
    return launch_rc(e);
}

// fe_step_chunk: fe_step(B, T) with the frames of each stream on the time pipeline.  work_dev: fe_pipe_layout(h, B, T).
static bool chunk_family(const fe_handle* h) { return h->cfg.arch == FE_ARCH_FASTENHANCER && h->impl && !h->d.BD; }

size_t fe_step_chunk_work_floats(const fe_handle* h, int B, int T) {
    if (!h || B <= 0 || T < 4 || !chunk_family(h)) return 0;
    return fe_pipe_layout(h, B, T).total;
}

// workgroups per stream of fe_step_chunk's pipelined launch (0: fe_step's own launch).  The second launch needs T H >= N - H: the new
// caches then hold nothing of the old ones.  T >= 4 implies it for every shipped shape but the hop-100 / n_fft-512 and hop-200 / n_fft-1024
// ones (FastEnhancer_L, dprnn L, 48 kHz L: N - H = 4.12 H): those pipeline from T = 5 on and walk at T = 4.
static int chunk_pipe_width(const fe_handle* h, int B, int T) {
    if (!chunk_family(h) || (long)T * h->d.HOP < h->d.NFFT - h->d.HOP) return 0;
    return pipe_width(h, B, T);
}

int fe_step_chunk(fe_handle* h, const float* wav_in_dev, size_t in_stride, float* state_dev, float* wav_out_dev, size_t out_stride, int B, int T,
                  float* work_dev, void* stream) {
    // fe_step's checks and refusals, the arguments first (as the pinned and packet steps check theirs)
    if (!h) return fail(FE_ERR_INVALID_ARG, "null handle");
    int rc = check_step_args(h, nullptr, "bad argument", wav_in_dev && state_dev && wav_out_dev, B, B, T, in_stride, out_stride);
    if (rc != FE_OK) return rc;
    if (h->cfg.arch == FE_ARCH_FASTENHANCER && h->d.BD) return fail(FE_ERR_UNSUPPORTED_CONFIG, "%s", kNoncausalNoStep);
    const int P = chunk_pipe_width(h, B, T);
    if (P == 0) return run_step(h, wav_in_dev, in_stride, state_dev, wav_out_dev, out_stride, B, T, nullptr, nullptr, stream);
    if (!work_dev) return fail(FE_ERR_INVALID_ARG, "fe_step_chunk: null work buffer (fe_step_chunk_work_floats(h, %d, %d) floats)", B, T);
    rc = check_ready(h);
    if (rc != FE_OK) return rc;
    KernelLogScope klog_(h);
    rc = ensure_scratch(h, B);
    if (rc != FE_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    const Dims& d = h->d;
    fe::StreamFrameArgs own{};
    own.capacity = B;
    const PipeLayout L = fe_pipe_layout(h, B, T);
    // (fe_step's own argument block, pointed at the work buffer)
    const fe::StreamFrameArgs a = pipe_args(fe_step_args(h, own, wav_in_dev, in_stride, state_dev, wav_out_dev, out_stride, B, T), work_dev, L, P);
    bool refused = false;
    rc = launch_pipe_carried(h, a, a.h, B, T, work_dev + L.ring, st, &refused);
    // the runtime refused co-residency (GPU shared with other work): walk the frames serially - fe_step's launch, made where fe_step makes it
    if (refused) return launch_fe_step(h, "fe_step", fe::STEP_PLAIN, own, wav_in_dev, in_stride, state_dev, wav_out_dev, out_stride, B, T, stream);
    if (rc != FE_OK) return rc;
    fe::note_kernel("stream_ola_kernel");
    hipLaunchKernelGGL(fe::stream_ola_kernel, dim3((T * d.HOP + fe::kThreads - 1) / fe::kThreads, B), dim3(fe::kThreads), 0, st,
                       a.frames, wav_in_dev, in_stride, a.cache_stft, a.cache_istft, wav_out_dev, out_stride, d.NFFT, d.HOP, T);
    return launch_rc(hipGetLastError());
}

// fe_step_backlog: fe_step(B, T) with the frames of each stream on the time pipeline, for every family that has a streaming state.
// FastEnhancer: fe_step_chunk.  The baseline families whose PIPE kernel hands the streaming state on in place (Fam::kPipeCarriesState:
// BSRNN, FSPEN), written once per family trait like baseline_offline: work_dev is pipe_layout(h, B, T, Fam::counters(h), 0) - sized for
// the pipelined launch whatever fe_set_time_pipeline says at the time of the query.
extern "C++" template <class Fam>
static PipeLayout baseline_backlog_layout(Fam, const fe_handle* h, int B, int T) {
    if (!Fam::kPipeCarriesState || !Fam::impl(h)->launch_pipe || B <= 0 || T < 4) return {0, 0, 0};
    return pipe_layout(h, B, T, Fam::counters(h), 0);
}

// A family whose PIPE kernel carries the streaming state only when asked (Fam::kPipeCarriesStateOnRequest: LiSenNet, under an explicit
// fe_set_time_pipeline(P >= 2)): that launch's work buffer - the counters, the windowed frames and the rings of the frames in flight, sized
// for the widest pipeline as baseline_layout sizes them.  A query of its own (fe_lisennet_backlog_work_floats): baseline_backlog_layout is 0.
extern "C++" template <class Fam>
static PipeLayout baseline_request_layout(Fam, const fe_handle* h, int B, int T) {
    if (!Fam::kPipeCarriesStateOnRequest || B <= 0 || T < 4) return {0, 0, 0};
    return pipe_layout(h, B, T, Fam::counters(h), (size_t)B * Fam::ring_floats(h));
}

// workgroups per stream of that launch (0: fe_step's own launch): an explicit width of two or more, a work buffer, a chunk that covers the
// overlap (stream_ola_kernel) - then what the family's fe_offline launch would take
extern "C++" template <class Fam>
static int baseline_request_width(Fam, const fe_handle* h, int B, int T, const float* work_dev) {
    if (!Fam::kPipeCarriesStateOnRequest || h->pipe_frames < 2 || !work_dev || (long)T * h->d.HOP < h->d.NFFT - h->d.HOP) return 0;
    return baseline_pipe_width(Fam{}, h, B, T);
}

// workgroups per stream of fe_step_backlog's pipelined launch: the family's fe_offline width (0: fe_step's own launch), and the chunk has
// to cover the overlap (stream_ola_kernel: T H >= N - H - every shipped BSRNN and FSPEN shape does at T = 4)
extern "C++" template <class Fam>
static int baseline_backlog_width(Fam, const fe_handle* h, int B, int T) {
    if (!Fam::kPipeCarriesState || (long)T * h->d.HOP < h->d.NFFT - h->d.HOP) return 0;
    return baseline_pipe_width(Fam{}, h, B, T);
}

// The pipelined chunk of a baseline family (P >= 2; the arguments are checked): a linear chain on the caller's stream - the counters'
// zeroing (a kernel, not a memset node: stft_kernels.hip.h), the family's cooperative PIPE kernel in streaming mode on the caller's state
// in place (not zeroed, not copied: frame 0 reads it, the last frame leaves the new one), stream_ola_kernel - that allocates nothing
// (Fam::args takes the per-family scratch the handle got at fe_load_weights, as baseline_offline does).  A cooperative launch the runtime
// refuses: fe_step's launch with the caller's own argument block - by then only the counters in work_dev have been written.
// REQ: the launch a family makes on request only (baseline_request_layout, with the rings; Fam::launch_pipe_stream) - the same chain.
extern "C++" template <class Fam, bool REQ = false>
static int baseline_step_backlog(Fam, fe_handle* h, const float* wav_in, size_t in_stride, float* state, float* wav_out, size_t out_stride, int B, int T, int P,
                                 float* work_dev, void* stream) {
    int rc = check_ready(h);
    if (rc != FE_OK) return rc;
    KernelLogScope klog_(h);
    hipStream_t st = (hipStream_t)stream;
    const Dims& d = h->d;
    typename Fam::StreamArgs a = Fam::args(h, B, T);
    Fam::state(a) = stream_io(a, wav_in, in_stride, wav_out, out_stride, state, state_layout(h, B));
    const PipeLayout L = REQ ? baseline_request_layout(Fam{}, h, B, T) : baseline_backlog_layout(Fam{}, h, B, T);
    typename Fam::Args p = pipe_args(a, work_dev, L, P);
    if constexpr (REQ) Fam::set_ring(p, work_dev + L.ring);
    const int nflags = (int)((size_t)B * Fam::counters(h));
    hipLaunchKernelGGL(fe::zero_counters_kernel, dim3((nflags + fe::kThreads - 1) / fe::kThreads), dim3(fe::kThreads), 0, st, p.pipe_flags, nflags);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return launch_rc(e);
    if constexpr (REQ) Fam::launch_pipe_stream(h, p, st, &e); else
    Fam::impl(h)->launch_pipe(p, st, &e);
    if (coop_refused(e)) {
        fe::g_klog.n = 0;       // (the refused launch was named before it was tried)
        return Fam::launch_step(h, a, fe::STEP_PLAIN, stream);
    }
    fe::note_kernel("stream_ola_kernel");
    hipLaunchKernelGGL(fe::stream_ola_kernel, dim3((T * d.HOP + fe::kThreads - 1) / fe::kThreads, B), dim3(fe::kThreads), 0, st,
                       p.frames, wav_in, in_stride, p.cache_stft, p.cache_istft, wav_out, out_stride, d.NFFT, d.HOP, T);
    return launch_rc(hipGetLastError());
}

size_t fe_step_backlog_work_floats(const fe_handle* h, int B, int T) {
    if (!h || B <= 0 || T < 4) return 0;
    size_t n = 0;
    if (visit_baseline(h->cfg.arch, [&](auto F) { n = baseline_backlog_layout(F, h, B, T).total; })) return n;
    return fe_step_chunk_work_floats(h, B, T);
}

int fe_step_backlog(fe_handle* h, const float* wav_in_dev, size_t in_stride, float* state_dev, float* wav_out_dev, size_t out_stride, int B, int T,
                    float* work_dev, void* stream) {
    if (!h) return fail(FE_ERR_INVALID_ARG, "null handle");
    if (h->cfg.arch == FE_ARCH_FASTENHANCER) return fe_step_chunk(h, wav_in_dev, in_stride, state_dev, wav_out_dev, out_stride, B, T, work_dev, stream);
    // fe_step's checks, the arguments first (as fe_step_chunk checks them)
    int rc = check_step_args(h, nullptr, "bad argument", wav_in_dev && state_dev && wav_out_dev, B, B, T, in_stride, out_stride);
    if (rc != FE_OK) return rc;
    int P = 0;
    visit_baseline(h->cfg.arch, [&](auto F) { P = baseline_backlog_width(F, h, B, T); });
    if (P == 0) {
        // a family that pipelines on request (LiSenNet): an explicit width >= 2 and a work buffer of fe_lisennet_backlog_work_floats
        bool done = false;
        visit_baseline(h->cfg.arch, [&](auto F) {
            using Fam = decltype(F);
            if constexpr (Fam::kPipeCarriesStateOnRequest) {
                if (const int Q = baseline_request_width(F, h, B, T, work_dev)) {
                    rc = baseline_step_backlog<Fam, true>(F, h, wav_in_dev, in_stride, state_dev, wav_out_dev, out_stride, B, T, Q, work_dev, stream);
                    done = true;
                }
            }
        });
        if (done) return rc;
        return run_step(h, wav_in_dev, in_stride, state_dev, wav_out_dev, out_stride, B, T, nullptr, nullptr, stream);
    }
    if (!work_dev) return fail(FE_ERR_INVALID_ARG, "fe_step_backlog: null work buffer (fe_step_backlog_work_floats(h, %d, %d) floats)", B, T);
    visit_baseline(h->cfg.arch, [&](auto F) { rc = baseline_step_backlog(F, h, wav_in_dev, in_stride, state_dev, wav_out_dev, out_stride, B, T, P, work_dev, stream); });
    return rc;
}

size_t fe_lisennet_backlog_work_floats(const fe_handle* h, int B, int T) {
    if (!h || B <= 0 || T < 4) return 0;
    size_t n = 0;
    visit_baseline(h->cfg.arch, [&](auto F) { n = baseline_request_layout(F, h, B, T).total; });
    return n;
}

// fe_step_pool_streams_chunk: fe_step_pool_streams_ctl with each stream's hops on the time pipeline, for every family with a streaming state.
// FastEnhancer: fe_step_streams_chunk (step_pool_streams hands the call over).  The baseline families whose PIPE kernel hands the streaming
// state on in place (Fam::kPipeCarriesState: BSRNN, FSPEN), written once over the family traits like baseline_step_backlog: work_dev is that
// call's layout, pipe_layout(h, n, T_max, Fam::counters(h), 0) - the size depends on the model, n and T_max only.  LiSenNet: 0 here - it
// pipelines on request (Fam::kPipeCarriesStateOnRequest), with the buffer of fe_lisennet_pool_streams_chunk_work_floats (below).
size_t fe_step_pool_streams_chunk_work_floats(const fe_handle* h, int n, int T_max) {
    if (!h || n <= 0 || T_max < 4) return 0;
    size_t floats = 0;
    if (visit_baseline(h->cfg.arch, [&](auto F) { floats = baseline_backlog_layout(F, h, n, T_max).total; })) return floats;
    return fe_step_streams_chunk_work_floats(h, n, T_max);
}

// workgroups per call stream of fe_step_pool_streams_chunk's pipelined launch: the family's fe_offline width for n streams of T_max frames
// (0: the packet step's own launch - T_max < 4, fe_set_time_pipeline(0 | 1), or too many streams to give each two co-resident workgroups).
// Any hop count 0 .. T_max is served on the pipeline - the host cannot see the descriptors - so there is no T H >= N - H condition here:
// stream_ola_streams_kernel orders its cache reads before its cache writes instead.
// A family whose pipeline carries the state on request only (Fam::kPipeCarriesStateOnRequest: LiSenNet) is pipelined on fe_step_backlog's
// terms: an explicit fe_set_time_pipeline(P >= 2) and a work buffer (fe_lisennet_pool_streams_chunk_work_floats) - without either the width
// is 0, and a null work buffer is no error.
static int pool_streams_chunk_pipe_width(const fe_handle* h, int n, int T_max, const float* work_dev) {
    int P = 0;
    if (n > 0) visit_baseline(h->cfg.arch, [&](auto F) {
        using Fam = decltype(F);
        if constexpr (Fam::kPipeCarriesState) P = baseline_pipe_width(F, h, n, T_max);
        else if constexpr (Fam::kPipeCarriesStateOnRequest) P = (h->pipe_frames >= 2 && work_dev) ? baseline_pipe_width(F, h, n, T_max) : 0;
    });
    return P;
}

// that launch's work buffer: fe_step_backlog's layout of the family - with the rings of the frames in flight where the family pipelines on request
extern "C++" template <class Fam>
static PipeLayout pool_streams_chunk_layout(Fam, const fe_handle* h, int n, int T_max) {
    return Fam::kPipeCarriesStateOnRequest ? baseline_request_layout(Fam{}, h, n, T_max) : baseline_backlog_layout(Fam{}, h, n, T_max);
}

size_t fe_lisennet_pool_streams_chunk_work_floats(const fe_handle* h, int n, int T_max) {
    if (!h || n <= 0 || T_max < 4) return 0;
    size_t floats = 0;
    visit_baseline(h->cfg.arch, [&](auto F) { floats = baseline_request_layout(F, h, n, T_max).total; });
    return floats;
}

// own: the packet step's fields as step_pool_streams has set them; wav_in / wav_out: device views.  A linear chain on the caller's stream - the
// counters' zeroing (stft_kernels.hip.h: a kernel, not a memset node), the family's cooperative PIPE + STRM frame kernel on the caller's state in
// place at each stream's slot, the audio kernel - that allocates nothing (Fam::args takes the per-family scratch the handle got at
// fe_load_weights, sized for a workgroup per CU, which bounds the cooperative grid).
// *refused: the runtime refused the cooperative launch; only the counters have been written.
static int launch_pool_streams_chunk(fe_handle* h, const BaselineStepOwn& own, const float* wav_in, float* state, float* wav_out, int n, int T_max, int P,
                                     float* work_dev, void* stream, bool* refused) {
    *refused = false;
    int rc = FE_OK;
    hipStream_t st = (hipStream_t)stream;
    visit_baseline(h->cfg.arch, [&](auto F) {
        using Fam = decltype(F);
        if constexpr (Fam::kPipeCarriesState || Fam::kPipeCarriesStateOnRequest) {
            typename Fam::StreamArgs a = Fam::args(h, n, T_max);
            a.capacity = own.capacity;
            static_cast<fe::StreamIoArgs&>(a) = own.io;
            Fam::state(a) = stream_io(a, wav_in, 0, wav_out, 0, state, state_layout(h, own.capacity));
            const PipeLayout L = pool_streams_chunk_layout(F, h, n, T_max);
            typename Fam::StreamArgs p = pipe_args(a, work_dev, L, P);
            Fam::set_ring(p, work_dev + L.ring);        // (a family without rings: nothing)
            const int nflags = (int)((size_t)n * Fam::counters(h));
            hipLaunchKernelGGL(fe::zero_counters_kernel, dim3((nflags + fe::kThreads - 1) / fe::kThreads), dim3(fe::kThreads), 0, st, p.pipe_flags, nflags);
            hipError_t e = hipGetLastError();
            if (e != hipSuccess) { rc = launch_rc(e); return; }
            if ((*refused = coop_refused(Fam::impl(h)->launch_streams_pipe(p, st)))) return;
            fe::note_kernel("stream_ola_streams_kernel");
            hipLaunchKernelGGL(fe::stream_ola_streams_kernel<typename Fam::StreamArgs>, dim3(n), dim3(fe::kThreads), 0, st, p, h->d.NFFT, h->d.HOP);
            rc = launch_rc(hipGetLastError());
        }
    });
    return rc;
}

int fe_step_pool_streams_chunk(fe_handle* h, const void* wav_in_dev, size_t in_count, float* state_dev, int capacity, const fe_stream_desc* desc_dev,
                               void* wav_out_dev, size_t out_count, int n, int T_max, int format, const float* min_gain, fe_stream_levels* levels,
                               float* work_dev, void* stream) {
    return step_pool_streams(h, "fe_step_pool_streams_chunk", false, wav_in_dev, in_count, state_dev, capacity, desc_dev, wav_out_dev, out_count, n, T_max,
                             format, stream, min_gain, levels, true, work_dev);
}

int fe_step_pool_streams_chunk_pinned(fe_handle* h, const void* wav_in_host, size_t in_count, float* state_dev, int capacity, const fe_stream_desc* desc_dev,
                                      void* wav_out_host, size_t out_count, int n, int T_max, int format, const float* min_gain, fe_stream_levels* levels,
                                      float* work_dev, void* stream) {
    return step_pool_streams(h, "fe_step_pool_streams_chunk_pinned", true, wav_in_host, in_count, state_dev, capacity, desc_dev, wav_out_host, out_count, n,
                             T_max, format, stream, min_gain, levels, true, work_dev);
}

// fe_step_streams_chunk: the packet step with each stream's hops on the time pipeline.  work_dev: fe_pipe_layout(h, n, T_max).  Built
// for the models whose frames exchange the GRU state only (default, ln, dprnn): the ring variants' ring_in_kernel /
// ring_out_kernel are not slotted, so time_kernel and dptransformer take the packet step itself, like every call the pipeline cannot take.
static bool streams_chunk_family(const fe_handle* h) { return chunk_family(h) && h->d.KT == 1 && !h->d.TA && h->impl->launch_streams_pipe != nullptr; }

size_t fe_step_streams_chunk_work_floats(const fe_handle* h, int n, int T_max) {
    if (!h || n <= 0 || T_max < 4 || !streams_chunk_family(h)) return 0;
    return fe_pipe_layout(h, n, T_max).total;
}

// workgroups per call stream of fe_step_streams_chunk's pipelined launch (0: the packet step's own launch).  Any hop count 0 .. T_max is
// served on the pipeline - the host cannot see the descriptors - so there is no T H >= N - H condition here: stream_ola_streams_kernel
// orders its cache reads before its cache writes instead.
static int streams_chunk_pipe_width(const fe_handle* h, int n, int T_max) {
    if (n <= 0 || !streams_chunk_family(h)) return 0;
    return pipe_width(h, n, T_max);
}

// own: the packet step's fields as step_streams has set them; wav_in / wav_out: device views.  A linear chain on the caller's stream - the
// counters' zeroing (stft_kernels.hip.h: a kernel, not a memset node), the cooperative frame kernel, the audio kernel - that allocates nothing
// (ensure_scratch allocated at fe_load_weights).
// *refused: the runtime refused the cooperative launch; only the counters have been written.
static int launch_streams_chunk(fe_handle* h, const fe::StreamFrameArgs& own, const float* wav_in, float* state, float* wav_out, int n, int T_max, int P,
                                float* work_dev, void* stream, bool* refused) {
    *refused = false;
    int rc = ensure_scratch(h, n);
    if (rc != FE_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    const fe::StreamFrameArgs a = pipe_args(fe_step_args(h, own, wav_in, 0, state, wav_out, 0, n, T_max), work_dev, fe_pipe_layout(h, n, T_max), P);
    const int nflags = (int)((size_t)n * pipe_counters(h));
    hipLaunchKernelGGL(fe::zero_counters_kernel, dim3((nflags + fe::kThreads - 1) / fe::kThreads), dim3(fe::kThreads), 0, st, a.pipe_flags, nflags);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return launch_rc(e);
    if ((*refused = coop_refused(h->impl->launch_streams_pipe(a, st)))) return FE_OK;
    h->last_shape = h->impl->name;
    fe::note_kernel("stream_ola_streams_kernel");
    hipLaunchKernelGGL(fe::stream_ola_streams_kernel<fe::StreamFrameArgs>, dim3(n), dim3(fe::kThreads), 0, st, a, h->d.NFFT, h->d.HOP);
    return launch_rc(hipGetLastError());
}

int fe_step_streams_chunk(fe_handle* h, const void* wav_in_dev, size_t in_count, float* state_dev, int capacity, const fe_stream_desc* desc_dev,
                          void* wav_out_dev, size_t out_count, int n, int T_max, int format, const float* min_gain, fe_stream_levels* levels,
                          const int* bank, float* work_dev, void* stream) {
    return step_streams(h, "fe_step_streams_chunk", false, wav_in_dev, in_count, state_dev, capacity, desc_dev, wav_out_dev, out_count, n, T_max, format,
                        stream, min_gain, levels, bank, true, work_dev);
}

int fe_step_streams_chunk_pinned(fe_handle* h, const void* wav_in_host, size_t in_count, float* state_dev, int capacity, const fe_stream_desc* desc_dev,
                                 void* wav_out_host, size_t out_count, int n, int T_max, int format, const float* min_gain, fe_stream_levels* levels,
                                 const int* bank, float* work_dev, void* stream) {
    return step_streams(h, "fe_step_streams_chunk_pinned", true, wav_in_host, in_count, state_dev, capacity, desc_dev, wav_out_host, out_count, n, T_max,
                        format, stream, min_gain, levels, bank, true, work_dev);
}

// The time-batched engine's schedule: one chain on the caller's stream, enc -> (scan k -> blk k) x KB -> dec, over all B x T frames of the
// call.  Only the scans are serial in time.  (Cutting the call into nodes over several streams, and a fused scan + tile stage, were
// measured and lost: profiles/r3d_tb_node_plans.txt, profiles/r3g_tb_fused_stage.txt.)
static int tb_run(fe_handle* h, fe::tb::TbArgs a, float* work_dev, int B, int T, hipStream_t st) {
    const Dims& d = h->d;
    const fe::tb::TbImpl* tbi = h->impl->tb;
    const TbLayout L = tb_layout(h, B, T);
#ifdef FE_TB_PROBE
    if (!h->tb_probe_dev) {
        FE_HIP_CHECK(hipMalloc(&h->tb_probe_dev, 4 * fe::tb::kProbeSlots * sizeof(unsigned long long)));
        FE_HIP_CHECK(hipMemset(h->tb_probe_dev, 0, 4 * fe::tb::kProbeSlots * sizeof(unsigned long long)));
    }
    a.probe = h->tb_probe_dev;
#endif
    a.B = B; a.T = T; a.NF = B * T;
    a.b0 = a.t0 = 0; a.Bfull = B; a.Tfull = T;
    a.h_init = (a.hstate != nullptr && a.h_init) ? 1 : 0;     // caches handed in (fe_spec_step): read by the scans, left updated
    a.xc = work_dev + L.xc;
    a.skip = work_dev + L.skip;
    a.x = work_dev + L.x;
    a.gx = work_dev + L.gx;
    a.hs = work_dev + L.hs;
    a.frames = work_dev + L.frames;
    if (a.NF == 0) return FE_OK;
    // (FE_TB_STAGES=n: stop after n launches - tools/gpu_tb_check.py reads the intermediate buffers out of work_dev)
    const char* lim_s = std::getenv("FE_TB_STAGES");
    int lim = lim_s ? std::atoi(lim_s) : 1 << 30;
    hipError_t e = hipSuccess;
    if (lim-- > 0) tbi->launch(fe::tb::TB_ENC, a, h->max_wgs, st, &e);
    for (int k = 0; k < d.KB && e == hipSuccess; ++k) {
        a.k = k;
        if (lim-- > 0) tbi->launch(fe::tb::TB_SCAN, a, h->max_wgs, st, &e);
        if (e == hipSuccess && lim-- > 0) tbi->launch(fe::tb::TB_BLK, a, h->max_wgs, st, &e);
    }
    if (e == hipSuccess && lim-- > 0) tbi->launch(fe::tb::TB_DEC, a, h->max_wgs, st, &e);
    return launch_rc(e);
}

// FE_OFFLINE_AUTO: the time-batched engine, except for the big shapes (M, L and their 48 kHz forms: block weights streamed from L2,
// one frame per tile) once there are enough utterances for the time-pipelined frame walk to fill the chip on its own - measured on
// FastEnhancer_L, 4 s: 1 utterance 5.2 ms time-batched / 14.2 ms walk, 16 utterances 20.6 / 16.8 ms (profiles/r3d_tb_timing.txt)
constexpr int kAutoWalkFrom = 8;
static bool use_tb_offline(const fe_handle* h, int B) {
    if (!h->impl || !h->impl->tb) return false;
    if (h->d.BD) return true;
    if (h->offline_engine == FE_OFFLINE_AUTO) return !(h->d.C2 >= 72 && B >= kAutoWalkFrom);
    return h->offline_engine != FE_OFFLINE_FRAME_WALK;
}

int fe_set_step_kernel(fe_handle* h, int kernel) {
    if (!h || kernel < FE_STEP_KERNEL_WAVES4 || kernel > FE_STEP_KERNEL_WG8_PERSIST) return fail(FE_ERR_INVALID_ARG, "bad argument");
    h->step_kernel = kernel;
    return FE_OK;
}

int fe_set_option(fe_handle* h, const char* name, int value) {
    if (!h || !name) return fail(FE_ERR_INVALID_ARG, "null argument");
    for (int i = 0; i < OPT_COUNT; ++i)
        if (std::strcmp(name, kOptions[i].name) == 0) {
            if (value < kOptions[i].lo || value > kOptions[i].hi)
                return fail(FE_ERR_INVALID_ARG, "fe_set_option(%s): %d is outside [%d, %d]", name, value, kOptions[i].lo, kOptions[i].hi);
            h->opt[i] = value;
            return FE_OK;
        }
    return fail(FE_ERR_INVALID_ARG, "fe_set_option: no option named '%s'", name);
}

int fe_get_option(const fe_handle* h, const char* name, int* value) {
    if (!h || !name || !value) return fail(FE_ERR_INVALID_ARG, "null argument");
    for (int i = 0; i < OPT_COUNT; ++i)
        if (std::strcmp(name, kOptions[i].name) == 0) { *value = h->opt[i]; return FE_OK; }
    return fail(FE_ERR_INVALID_ARG, "fe_get_option: no option named '%s'", name);
}

int fe_options(void) { return OPT_COUNT; }
const char* fe_option_name(int idx) { return idx >= 0 && idx < OPT_COUNT ? kOptions[idx].name : nullptr; }

const char* fe_last_step_kernel(const fe_handle* h) {
    if (!h) return "";
    std::string& s = h->last_text;
    s.clear();
    const int n = h->n_last_kernels < 16 ? h->n_last_kernels : 16;
    for (int i = 0; i < n;) {
        int j = i;
        while (j < n && h->last_kernels[j] == h->last_kernels[i]) ++j;
        if (!s.empty()) s += " + ";
        if (j - i > 1) s += std::to_string(j - i) + " x ";
        s += h->last_kernels[i];
        i = j;
    }
    if (h->n_last_kernels > 16) s += " + ...";
    if (!s.empty() && h->last_shape) s += std::string(" [shape ") + h->last_shape + "]";
    return s.c_str();
}

int fe_set_offline_engine(fe_handle* h, int engine) {
    if (!h || engine < FE_OFFLINE_AUTO || engine > FE_OFFLINE_TIME_BATCHED) return fail(FE_ERR_INVALID_ARG, "bad argument");
    if (engine == FE_OFFLINE_TIME_BATCHED && !(h->impl && h->impl->tb)) return fail(FE_ERR_UNSUPPORTED_CONFIG, "no time-batched engine is compiled for this model");
    if (engine == FE_OFFLINE_FRAME_WALK && h->d.BD) return fail(FE_ERR_UNSUPPORTED_CONFIG, "the noncausal model runs on the time-batched engine only");
    h->offline_engine = engine;
    return FE_OK;
}

// fe_offline on the time-batched engine: encoder pass, per block (scan over time, attention pass), decoder pass, overlap-add.
// Tw_b_dev != nullptr: a ragged batch laid out for Tw (= the longest utterance), utterance b has Tw_b_dev[b] samples.
static int offline_tb(fe_handle* h, const float* noisy_dev, size_t in_stride, const int* Tw_b_dev, int Tw, int B, float* wav_hat_dev, size_t out_stride,
                      float* spec_hat_dev, float* work_dev, hipStream_t st) {
    const Dims& d = h->d;
    const int T = 1 + Tw / d.HOP;
    int rc = ensure_tables(h, st);
    if (rc != FE_OK) return rc;
    fe::tb::TbArgs a{};
    a.wp = h->packed_dev;
    a.wav_in = noisy_dev; a.in_stride = in_stride; a.Tw = Tw; a.Tw_b = Tw_b_dev;
    a.spec_out = spec_hat_dev;
    a.hstate = nullptr;                      // zero initial state (model.py:626-627)
    a.mode = fe::FE_MODE_OFFLINE;
    a.compression = h->cfg.input_compression;
    rc = tb_run(h, a, work_dev, B, T, st);
    if (rc != FE_OK) return rc;
    return ola(h, work_dev + tb_layout(h, B, T).frames, wav_hat_dev, out_stride, B, T, st, Tw_b_dev);
}

size_t fe_offline_work_floats(const fe_handle* h, int B, int Tw) {
    if (!h || B <= 0 || Tw <= 0) return 0;
    const Dims& d = h->d;
    const int T = 1 + Tw / d.HOP;
    size_t n = 0;
    if (visit_baseline(h->cfg.arch, [&](auto F) { n = baseline_layout(F, h, B, T).total; })) return n;
    // FastEnhancer.  The frame walk's buffer with the pipeline's region, whatever fe_set_time_pipeline says at the time of THIS call: a
    // buffer sized with the pipeline off must still do when it is on.  (The shapes with a time-batched engine include the region for every
    // T, the others from the pipeline's 4 frames on: the sizes callers have been given, pinned by tests/golden/host_queries.json.)
    const OfflineLayout L = fe_walk_layout(h, B, T);
    const size_t walk = d.BD ? 0 : (h->impl->tb || T >= 4) ? L.total : L.pipe;
    if (!h->impl->tb) return walk;
    // Sized for the engine the CURRENT fe_set_offline_engine setting selects (FastEnhancer_L x 16 x 4 s: the time-batched buffers are
    // 3 GB against the frame walk's 25 MB), and MONOTONE in B under that setting: a buffer sized for B serves every batch of at most B
    // utterances of at most Tw samples.  Under AUTO the big shapes walk from 8 utterances on but take the time-batched engine below
    // that, so their size covers the time-batched need of min(B, 7) as well.  After fe_set_offline_engine: query again (header).
    if (d.BD || use_tb_offline(h, B)) return std::max(walk, tb_layout(h, B, T).total);
    if (h->offline_engine == FE_OFFLINE_AUTO) return std::max(walk, tb_layout(h, std::min(B, kAutoWalkFrom - 1), T).total);
    return walk;
}

int fe_offline(fe_handle* h, const float* noisy_dev, int B, int Tw, float* wav_hat_dev, float* spec_hat_dev, float* work_dev,
               void* stream) {
    int rc = check_ready(h);
    if (rc != FE_OK) return rc;
    KernelLogScope klog_(h);
    if (!noisy_dev || !wav_hat_dev || !spec_hat_dev || !work_dev || B <= 0) return fail(FE_ERR_INVALID_ARG, "bad argument");
    const Dims& d = h->d;
    if (Tw <= d.NFFT / 2)   // torch.stft reflect padding needs pad < length
        return fail(FE_ERR_INVALID_ARG, "Tw=%d: reflect padding of n_fft/2=%d needs a longer input", Tw, d.NFFT / 2);
    hipStream_t st = (hipStream_t)stream;
    if (visit_baseline(h->cfg.arch, [&](auto F) { rc = baseline_offline(F, h, noisy_dev, B, Tw, wav_hat_dev, spec_hat_dev, work_dev, st); })) return rc;
    const int T = 1 + Tw / d.HOP;
    if (use_tb_offline(h, B)) return offline_tb(h, noisy_dev, (size_t)Tw, nullptr, Tw, B, wav_hat_dev, (size_t)d.HOP * (T - 1), spec_hat_dev, work_dev, st);
    const OfflineLayout L = fe_walk_layout(h, B, T);
    const int P = pipe_width(h, B, T);
    // zero the tail and the state (zero initial state, model.py:626-627), and the frame counters of a pipelined launch
    FE_HIP_CHECK(hipMemsetAsync(work_dev, 0, (L.pipe + (P ? L.p.frames : 0)) * sizeof(float), st));
    rc = ensure_scratch(h, B);
    if (rc != FE_OK) return rc;
    fe::StreamFrameArgs a = base_args(h, B, T);
    a.mode = fe::FE_MODE_OFFLINE;
    a.Tw = Tw;
    a.wav_in = noisy_dev;
    a.in_stride = (size_t)Tw;
    a.wav_out = wav_hat_dev;
    a.out_stride = (size_t)d.HOP * (T - 1);
    a.spec_out = spec_hat_dev;
    a.cache_istft = work_dev;
    a.cache_stft = work_dev;   // unused in this mode
    a.h = work_dev + L.state;
    a.tk = a.h + (size_t)B * d.hstate();
    hipError_t e = hipSuccess;
    if (P) {
        rc = ensure_tables(h, st);
        if (rc != FE_OK) return rc;
        fe::StreamFrameArgs p = pipe_args(a, work_dev + L.pipe, L.p, P);
        if (d.KT > 1) p.tk = work_dev + L.pipe + L.p.ring;      // (PIPE: rings of P + KT - 1 slots per conv and stream)
        if (d.TA) p.h = work_dev + L.pipe + L.p.ring;           // (PIPE: K / V rings of L + P slots per pair)
        h->impl->launch_pipe(p, st, &e);
        if (!coop_refused(e)) return ola(h, p.frames, wav_hat_dev, a.out_stride, B, T, st);
        // the runtime refused co-residency (GPU shared with other work): walk the frames serially
    }
    h->impl->launch_step(a, fe::STEP_PLAIN, h->max_wgs, st, &e);
    return launch_rc(e);
}

// ---------------------------------------------------------------------------- stand-alone STFT / iSTFT
static int ensure_tables(fe_handle* h, hipStream_t st) {
    if (h->tables_dev) return FE_OK;
    const size_t N = (size_t)h->cfg.n_fft;
    std::vector<float> t(3 * N);
    memcpy(&t[0], h->window.data(), N * sizeof(float));
    memcpy(&t[N], h->window_istft.data(), N * sizeof(float));
    memcpy(&t[2 * N], h->twiddle.data(), N * sizeof(float));
    FE_HIP_CHECK(hipMalloc(&h->tables_dev, 3 * N * sizeof(float)));
    FE_HIP_CHECK(hipMemcpyAsync(h->tables_dev, t.data(), 3 * N * sizeof(float), hipMemcpyHostToDevice, st));
    FE_HIP_CHECK(hipStreamSynchronize(st));
    return FE_OK;
}

#define FE_STFT_LAUNCH(kernel, a, grid, st)                                                         \
    do {                                                                                            \
        if (h->cfg.n_fft == 512) hipLaunchKernelGGL((fe::kernel<512>), grid, dim3(fe::kThreads), 0, st, a);        \
        else if (h->cfg.n_fft == 1024) hipLaunchKernelGGL((fe::kernel<1024>), grid, dim3(fe::kThreads), 0, st, a); \
        else return fail(FE_ERR_UNSUPPORTED_CONFIG, "n_fft=%d (stand-alone STFT kernels: 512, 1024)", h->cfg.n_fft); \
        hipError_t e_ = hipGetLastError();                                                          \
        if (e_ != hipSuccess) return fail(FE_ERR_HIP, "kernel launch: %s", hipGetErrorString(e_));  \
    } while (0)

static fe::StftArgs stft_args(const fe_handle* h, int B) {
    fe::StftArgs a{};
    a.tables = h->tables_dev;
    a.B = B;
    a.T = 1;
    a.H = h->cfg.hop_size;
    a.compression = 1.0f;
    a.eps = 1.0e-5f;
    return a;
}

// spec_hat rows of an offline call: N/2 (FastEnhancer: the model drops the Nyquist bin) or N/2 + 1 (BSRNN / FSPEN / LiSenNet)
static int offline_spec_rows(const fe_handle* h) { return h->d.NFFT / 2 + (h->cfg.arch == FE_ARCH_FASTENHANCER ? 0 : 1); }

// A ragged batch has ONE batched form: the time-batched engine (the frame walk and its time pipeline take one length per launch).  It is
// taken whenever the model has that engine and the caller has not asked for the frame walk - also for the big shapes at 8+ utterances,
// where AUTO would walk an equal-length batch: sixteen 4 s files of FastEnhancer_L are 20.6 ms in one time-batched pass, 16 x 5.2 ms one by one.
static bool ragged_uses_tb(const fe_handle* h) {
    return h->impl && h->impl->tb && (h->d.BD || h->offline_engine != FE_OFFLINE_FRAME_WALK);
}

// scratch of the call's engine: the batched pass, or the one-by-one fallback's largest single call (fe_offline_work_floats is monotone in B)
static size_t ragged_base_floats(const fe_handle* h, int B, int Tw_max) {
    if (ragged_uses_tb(h)) return tb_layout(h, B, 1 + Tw_max / h->d.HOP).total;
    return std::max(fe_offline_work_floats(h, B, Tw_max), fe_offline_work_floats(h, 1, Tw_max));
}

size_t fe_offline_ragged_work_floats(const fe_handle* h, int B, int Tw_max) {
    if (!h || B <= 0 || Tw_max <= 0) return 0;
    const int Tmax = 1 + Tw_max / h->d.HOP;
    // the call's scratch, the per-utterance lengths, one utterance's spec_hat (the one-by-one fallback)
    return ragged_base_floats(h, B, Tw_max) + round4((size_t)B) + (size_t)offline_spec_rows(h) * Tmax * 2;
}

int fe_offline_ragged(fe_handle* h, const float* noisy_dev, size_t in_stride, const int* Tw_host, int B, float* wav_hat_dev, size_t out_stride,
                      float* spec_hat_dev, float* work_dev, void* stream) {
    int rc = check_ready(h);
    if (rc != FE_OK) return rc;
    KernelLogScope klog_(h);
    if (!noisy_dev || !Tw_host || !wav_hat_dev || !spec_hat_dev || !work_dev || B <= 0) return fail(FE_ERR_INVALID_ARG, "bad argument");
    const Dims& d = h->d;
    int Tw_max = 0;
    for (int b = 0; b < B; ++b) {
        if (Tw_host[b] <= d.NFFT / 2) return fail(FE_ERR_INVALID_ARG, "Tw[%d]=%d: reflect padding of n_fft/2=%d needs a longer input", b, Tw_host[b], d.NFFT / 2);
        if ((size_t)Tw_host[b] > in_stride && B > 1) return fail(FE_ERR_INVALID_ARG, "Tw[%d]=%d > in_stride %zu", b, Tw_host[b], in_stride);
        Tw_max = std::max(Tw_max, Tw_host[b]);
    }
    const int Tmax = 1 + Tw_max / d.HOP;
    if (out_stride < (size_t)d.HOP * (Tmax - 1) && B > 1) return fail(FE_ERR_INVALID_ARG, "out_stride %zu < H*(Tmax-1)", out_stride);
    hipStream_t st = (hipStream_t)stream;
    const size_t base = ragged_base_floats(h, B, Tw_max);
    if (ragged_uses_tb(h)) {
        // ONE batched call laid out for the longest utterance; every utterance's frames past its own end are computed on clamped input and
        // stay out of its output (causal in time; the noncausal model's reverse scans start at each utterance's own last frame)
        int* Tw_dev = reinterpret_cast<int*>(work_dev + base);
        FE_HIP_CHECK(hipMemcpyAsync(Tw_dev, Tw_host, (size_t)B * sizeof(int), hipMemcpyHostToDevice, st));
        return offline_tb(h, noisy_dev, in_stride, Tw_dev, Tw_max, B, wav_hat_dev, out_stride, spec_hat_dev, work_dev, st);
    }
    // no batched form for this model / engine setting (the frame walk and its time pipeline take ONE length per launch): one by one
    const int F = offline_spec_rows(h);
    float* spec_tmp = work_dev + base + round4((size_t)B);
    for (int b = 0; b < B; ++b) {
        const int Tb = 1 + Tw_host[b] / d.HOP;
        float* dst = spec_hat_dev + (size_t)b * F * Tmax * 2;
        rc = fe_offline(h, noisy_dev + (size_t)b * in_stride, 1, Tw_host[b], wav_hat_dev + (size_t)b * out_stride, Tb == Tmax ? dst : spec_tmp, work_dev, stream);
        if (rc != FE_OK) return rc;
        if (Tb != Tmax)
            FE_HIP_CHECK(hipMemcpy2DAsync(dst, (size_t)Tmax * 2 * sizeof(float), spec_tmp, (size_t)Tb * 2 * sizeof(float), (size_t)Tb * 2 * sizeof(float), (size_t)F,
                                          hipMemcpyDeviceToDevice, st));
    }
    return FE_OK;
}

int fe_stft_step(fe_handle* h, const float* wav_in_dev, size_t in_stride, const float* cache_in_dev, float* cache_out_dev,
                 float* spec_out_dev, int B, void* stream) {
    if (!h || !wav_in_dev || !cache_in_dev || !cache_out_dev || !spec_out_dev || B <= 0) return fail(FE_ERR_INVALID_ARG, "bad argument");
    hipStream_t st = (hipStream_t)stream;
    int rc = ensure_tables(h, st);
    if (rc != FE_OK) return rc;
    fe::StftArgs a = stft_args(h, B);
    a.wav_in = wav_in_dev; a.in_stride = in_stride; a.cache_in = cache_in_dev; a.cache_out = cache_out_dev; a.spec = spec_out_dev;
    FE_STFT_LAUNCH(stft_step_kernel, a, dim3(B), st);
    return FE_OK;
}

int fe_istft_step(fe_handle* h, const float* spec_in_dev, const float* cache_in_dev, float* cache_out_dev, float* wav_out_dev,
                  size_t out_stride, int B, void* stream) {
    if (!h || !spec_in_dev || !cache_in_dev || !cache_out_dev || !wav_out_dev || B <= 0) return fail(FE_ERR_INVALID_ARG, "bad argument");
    hipStream_t st = (hipStream_t)stream;
    int rc = ensure_tables(h, st);
    if (rc != FE_OK) return rc;
    fe::StftArgs a = stft_args(h, B);
    a.spec = const_cast<float*>(spec_in_dev); a.cache_in = cache_in_dev; a.cache_out = cache_out_dev;
    a.wav_out = wav_out_dev; a.out_stride = out_stride;
    FE_STFT_LAUNCH(istft_step_kernel, a, dim3(B), st);
    return FE_OK;
}

int fe_stft_offline(fe_handle* h, const float* noisy_dev, int B, int Tw, int F, int compress, float* spec_out_dev, void* stream) {
    if (!h || !noisy_dev || !spec_out_dev || B <= 0) return fail(FE_ERR_INVALID_ARG, "bad argument");
    const int N = h->cfg.n_fft, H = h->cfg.hop_size;
    if (Tw <= N / 2) return fail(FE_ERR_INVALID_ARG, "Tw=%d: reflect padding of n_fft/2=%d needs a longer input", Tw, N / 2);
    if (F != N / 2 && F != N / 2 + 1) return fail(FE_ERR_INVALID_ARG, "F=%d (n_fft/2 or n_fft/2+1)", F);
    hipStream_t st = (hipStream_t)stream;
    int rc = ensure_tables(h, st);
    if (rc != FE_OK) return rc;
    fe::StftArgs a = stft_args(h, B);
    a.T = 1 + Tw / H; a.Tw = Tw; a.F = F;
    a.wav_in = noisy_dev; a.in_stride = (size_t)Tw; a.spec = spec_out_dev;
    a.compression = compress ? h->cfg.input_compression : 1.0f;
    FE_STFT_LAUNCH(stft_frames_kernel, a, dim3(a.T, B), st);
    return FE_OK;
}

int fe_istft_offline(fe_handle* h, const float* spec_in_dev, int B, int T, int F, int compress, float* wav_out_dev,
                     float* frames_dev, void* stream) {
    if (!h || !spec_in_dev || !wav_out_dev || !frames_dev || B <= 0 || T <= 1) return fail(FE_ERR_INVALID_ARG, "bad argument");
    const int N = h->cfg.n_fft, H = h->cfg.hop_size;
    if (F != N / 2 && F != N / 2 + 1) return fail(FE_ERR_INVALID_ARG, "F=%d (n_fft/2 or n_fft/2+1)", F);
    hipStream_t st = (hipStream_t)stream;
    int rc = ensure_tables(h, st);
    if (rc != FE_OK) return rc;
    fe::StftArgs a = stft_args(h, B);
    a.T = T; a.F = F;
    a.spec = const_cast<float*>(spec_in_dev); a.frames = frames_dev;
    a.compression = compress ? h->cfg.input_compression : 1.0f;
    FE_STFT_LAUNCH(istft_frames_kernel, a, dim3(T, B), st);
    return ola(h, frames_dev, wav_out_dev, (size_t)H * (T - 1), B, T, st);
}

double fe_flops_per_frame(const fe_handle* h) {
    if (!h) return 0.0;
    const Dims& d = h->d;
    double macs = 0;
    if (visit_baseline(h->cfg.arch, [&](auto F) { macs = F.macs(h); })) return 2.0 * macs + 2.0 * 2.5 * d.NFFT * std::log2((double)d.NFFT);
    const double C1 = d.C1, C2 = d.C2, F1 = d.F1, F2 = d.F2, K = d.KB;
    const double KT = d.KT;
    double m = 2 * C1 * 8 * F1;
    for (int i = 1; i <= d.NL; ++i) m += C1 * C1 * 3 * KT * F1;
    m += F1 * F2 * C1 + C1 * C2 * F2;
    if (d.TA) m += K * (C2 * C2 * 3 * F2 + 2 * (d.TA + 1) * C2 * F2 + C2 * C2 * F2 + C2 * C2 * 3 * F2 + 2 * F2 * C2 * F2 + C2 * C2 * F2);
    else if (d.FR) {  // time GRU + fc, then the sub-band GRU (input and hidden products of both directions) + fc
        const double H = C2 / 2;
        m += K * (C2 * C2 * 6 * F2 + C2 * C2 * F2 + 2 * 3 * H * (C2 + H) * F2 + 2 * H * C2 * F2);
    } else if (d.BD)  // both GRU directions, rnn_fc over 2 C2
    m += K * (2 * C2 * C2 * 6 * F2 + 2 * C2 * C2 * F2 + C2 * C2 * 3 * F2 + 2 * F2 * C2 * F2 + C2 * C2 * F2);
    else
    m += K * (C2 * C2 * 6 * F2 + C2 * C2 * F2 + C2 * C2 * 3 * F2 + 2 * F2 * C2 * F2 + C2 * C2 * F2);
    m += F2 * F1 * C2 + C2 * C1 * F1;
    for (int i = 1; i <= d.NL; ++i) m += 2 * C1 * C1 * F1 + C1 * C1 * 3 * KT * F1;
    m += 2 * C1 * C1 * F1 + C1 * 2 * 8 * F1;
    return 2.0 * m + 2.0 * 2.5 * d.NFFT * std::log2((double)d.NFFT);
}

int fe_debug_stages(const fe_handle* h) {
    if (!h) return 0;
    int n = h->impl ? h->impl->dbg_stages : 0;
    visit_baseline(h->cfg.arch, [&](auto F) { n = F.impl(h)->dbg_stages; });
    return n;
}

size_t fe_debug_floats(const fe_handle* h) {
    if (!h) return 0;
    size_t n = h->impl ? h->impl->dbg_floats : 0;
    visit_baseline(h->cfg.arch, [&](auto F) { n = F.impl(h)->dbg_floats; });
    return n;
}

int fe_debug_stage(const fe_handle* h, int idx, const char** name, int* rows, int* cols, size_t* offset_floats) {
    if (!h || idx < 0 || idx >= fe_debug_stages(h)) return fail(FE_ERR_INVALID_ARG, "stage index %d", idx);
    int r, c;
    size_t off;
    const char* stage = nullptr;
    if (!visit_baseline(h->cfg.arch, [&](auto F) { stage = F.stage_name(h, idx); F.impl(h)->dbg_stage(idx, &r, &c, &off); })) {
        static thread_local std::string nm;
        const Dims& d = h->d;
        char buf[64];
        int s = idx;
        if (s == 0) nm = "spec_in";
        else if (s == 1) nm = "compressed";
        else if (s == 2) nm = "enc_pre";
        else if (s < 3 + d.NL) { snprintf(buf, sizeof buf, "encoder.%d", s - 3); nm = buf; }
        else if (s == 3 + d.NL) nm = "rf_pre";
        else if (s < 4 + d.NL + 2 * d.KB) {
            int k = (s - 4 - d.NL) / 2, w = (s - 4 - d.NL) % 2;
            snprintf(buf, sizeof buf, w == 0 ? "rf_block.%d.rnn" : "rf_block.%d", k); nm = buf;
        } else if (s == 4 + d.NL + 2 * d.KB) nm = "rf_post";
        else if (s < 5 + 2 * d.NL + 2 * d.KB) { snprintf(buf, sizeof buf, "decoder.%d", s - 5 - d.NL - 2 * d.KB); nm = buf; }
        else if (s == 5 + 2 * d.NL + 2 * d.KB) nm = "mask";
        else nm = "spec_out";
        stage = nm.c_str();
        h->impl->dbg_stage(idx, &r, &c, &off);
    }
    if (name) *name = stage;
    if (rows) *rows = r;
    if (cols) *cols = c;
    if (offset_floats) *offset_floats = off;
    return FE_OK;
}

}  // extern "C"

// the polyphase resampler: a handle of its own (fe_resampler), no model behind it
#include "fe_api_resample.inc"
