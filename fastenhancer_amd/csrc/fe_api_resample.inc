// fe_api_resample.inc — the host side of the polyphase resampler (fe_resampler_*, fe_resample, fe_resample_streams[_pinned],
// fe_resample_rings[_pinned]): the filter
// design, the index arithmetic of the contract (include/fastenhancer_hip.h, "Audio at another sample rate"), the argument checks and the
// launches of resample_kernels.hip.h (through fe::launch_resample of fe_resample.hip, where the kernels are compiled).  Included by fe_api.hip at file scope, behind the model handle's entry points (it uses their fail,
// pinned_view and table_view).

struct fe_resampler {
    int sr_in = 0, sr_out = 0;
    int up = 0, down = 0, hl = 0, K = 0, KP = 0;
    int tile_out = 0, xcap = 0;
    size_t lds_bytes = 0;
    std::vector<double> taps;          // h[L], as designed
    std::vector<float> table;          // [up][KP], T[r][j] = (float)h[r + j up], 0 past the last tap
    float* table_dev = nullptr;        // uploaded by the first launch
    int device = -1;
    const char* last_kernel = "";
};

namespace {

constexpr int kResampleMaxRatio = 640;
constexpr int kResampleTileOut = 1024;       // outputs per tile at most ...
constexpr int kResampleTileIn = 4096;        // ... and input samples a tile advances at most
// workgroups of one launch: a HIP launch takes fewer than 2^32 threads in all, and a workgroup has 256
constexpr long long kResampleMaxWorkgroups = 0xffffffffll / fe::kResampleThreads;

static_assert(sizeof(fe_resample_desc) == 24 && sizeof(fe::ResampleDesc) == 24 && offsetof(fe_resample_desc, slot) == offsetof(fe::ResampleDesc, slot) &&
              offsetof(fe_resample_desc, n_in) == offsetof(fe::ResampleDesc, n_in) && offsetof(fe_resample_desc, in_offset) == offsetof(fe::ResampleDesc, in_offset) &&
              offsetof(fe_resample_desc, out_offset) == offsetof(fe::ResampleDesc, out_offset), "fe_resample_desc is the kernel's ResampleDesc");
static_assert(sizeof(fe_resample_ring_desc) == 40 && sizeof(fe::ResampleRingDesc) == 40 && offsetof(fe_resample_ring_desc, slot) == offsetof(fe::ResampleRingDesc, slot) &&
              offsetof(fe_resample_ring_desc, n_in) == offsetof(fe::ResampleRingDesc, n_in) && offsetof(fe_resample_ring_desc, in_base) == offsetof(fe::ResampleRingDesc, in_base) &&
              offsetof(fe_resample_ring_desc, out_base) == offsetof(fe::ResampleRingDesc, out_base) && offsetof(fe_resample_ring_desc, in_len) == offsetof(fe::ResampleRingDesc, in_len) &&
              offsetof(fe_resample_ring_desc, in_pos) == offsetof(fe::ResampleRingDesc, in_pos) && offsetof(fe_resample_ring_desc, out_len) == offsetof(fe::ResampleRingDesc, out_len) &&
              offsetof(fe_resample_ring_desc, out_pos) == offsetof(fe::ResampleRingDesc, out_pos), "fe_resample_ring_desc is the kernel's ResampleRingDesc");

// modified Bessel function I0 by its power series (every term positive: relative error of a few ulp for the arguments 0 .. 5 used here)
double bessel_i0(double x) {
    const double q = 0.25 * x * x;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 64; ++k) {
        term *= q / ((double)k * (double)k);
        sum += term;
        if (term < 1e-20 * sum) break;
    }
    return sum;
}

long long resample_gcd(long long a, long long b) {
    while (b) { const long long t = a % b; a = b; b = t; }
    return a;
}

// M(N): outputs emitted after N consumed samples
long long resample_emitted(const fe_resampler* rs, long long N) {
    const long long a = N * rs->up - rs->hl;
    return a > 0 ? (a + rs->down - 1) / rs->down : 0;
}

static_assert(FE_AUDIO_ULAW == fe::kAudioUlaw && FE_AUDIO_ALAW == fe::kAudioAlaw, "the G.711 format codes are the kernel's");

bool resample_is_g711(int format) { return format == FE_AUDIO_ULAW || format == FE_AUDIO_ALAW; }

int resample_check_format(const char* fn, const char* what, int format) {
    if (format != FE_AUDIO_F32 && format != FE_AUDIO_S16 && !resample_is_g711(format))
        return fail(FE_ERR_INVALID_ARG, "%s: %s %d is neither FE_AUDIO_F32 (0) nor FE_AUDIO_S16 (1), nor FE_AUDIO_ULAW (4) or FE_AUDIO_ALAW (5)", fn, what,
                    format);
    return FE_OK;
}

// the page-locked range lookup for a buffer of `format`: elements of 4, 2 or 1 bytes
auto resample_pinned_view(int format) -> int (*)(const void*, size_t, const char*, const char*, const void**) {
    if (resample_is_g711(format)) return &pinned_view<unsigned char>;
    return format == FE_AUDIO_S16 ? &pinned_view<short> : &pinned_view<float>;
}

// the first launch of a handle: the tap table goes to the current device
int resample_ensure_table(fe_resampler* rs, const char* fn) {
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess) {
        (void)hipGetLastError();
        return fail(FE_ERR_HIP, "%s: no HIP device (the resampler runs on the GPU: there is no CPU fallback)", fn);
    }
    if (rs->table_dev) {
        if (dev != rs->device)
            return fail(FE_ERR_INVALID_ARG, "%s: the resampler's tap table lives on device %d, the current device is %d", fn, rs->device, dev);
        return FE_OK;
    }
    float* p = nullptr;
    FE_HIP_CHECK(hipMalloc(&p, rs->table.size() * sizeof(float)));
    const hipError_t e = hipMemcpy(p, rs->table.data(), rs->table.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(p);
        return fail(FE_ERR_HIP, "%s: uploading the tap table: %s", fn, hipGetErrorString(e));
    }
    rs->table_dev = p;
    rs->device = dev;
    return FE_OK;
}

fe::ResampleArgs resample_args(const fe_resampler* rs, const void* in, int in_format, void* out, int out_format) {
    fe::ResampleArgs a{};
    a.table = rs->table_dev;
    a.up = rs->up; a.down = rs->down; a.hl = rs->hl; a.K = rs->K; a.KP = rs->KP;
    a.tile_out = rs->tile_out; a.xcap = rs->xcap;
    a.in = in; a.out = out;
    a.in_format = in_format; a.out_format = out_format;
    return a;
}

// fe_resample_streams[_pinned] (Desc = fe_resample_desc) and fe_resample_rings[_pinned] (fe_resample_ring_desc): one set of checks, in one
// order, with one set of texts; the descriptor type picks the argument block, the launcher and the kernel's name
template <class Desc>
int resample_streams(fe_resampler* rs, const char* fn, bool pinned, const void* in, size_t in_count, int in_format, float* state_dev, int capacity,
                     const Desc* desc_dev, void* out, size_t out_count, int out_format, int* produced, int n, int n_in_max, void* stream) {
    constexpr bool RING = std::is_same<Desc, fe_resample_ring_desc>::value;
    if (!rs) return fail(FE_ERR_INVALID_ARG, "%s: null resampler", fn);
    if (!in || !state_dev || !desc_dev || !out || n <= 0 || n_in_max <= 0 || capacity < n || in_count == 0 || out_count == 0)
        return fail(FE_ERR_INVALID_ARG, "%s: bad argument (need non-null pointers to at least one element, 1 <= n <= capacity, n_in_max >= 1)", fn);
    int rc = resample_check_format(fn, "in_format", in_format);
    if (rc == FE_OK) rc = resample_check_format(fn, "out_format", out_format);
    if (rc != FE_OK) return rc;
    if (n > kResampleMaxWorkgroups) return fail(FE_ERR_INVALID_ARG, "%s: %d streams exceed the launch grid (%lld: split the call)", fn, n, kResampleMaxWorkgroups);
    if ((long long)n_in_max * rs->up / rs->down + 1 > 0x7fffffffll)
        return fail(FE_ERR_INVALID_ARG, "%s: n_in_max %d: a stream's output count would not fit the int table `produced`", fn, n_in_max);
    const void* in_v = in;
    const void* out_v = out;
    if (pinned) {
        const auto vin = resample_pinned_view(in_format), vout = resample_pinned_view(out_format);
        rc = vin(in, in_count, fn, "in", &in_v);
        if (rc == FE_OK) rc = vout(out, out_count, fn, "out", &out_v);
        if (rc != FE_OK) return rc;
    }
    const void* prod_v = nullptr;
    rc = table_view(produced, (size_t)n * sizeof(int), fn, "produced", &prod_v);
    if (rc == FE_OK) rc = resample_ensure_table(rs, fn);
    if (rc != FE_OK) return rc;
    typename fe::ResampleKernelArgs<RING>::type a{};
    static_cast<fe::ResampleArgs&>(a) = resample_args(rs, in_v, in_format, const_cast<void*>(out_v), out_format);
    a.n_in_max = n_in_max;
    a.in_count = in_count; a.out_count = out_count;
    a.state = state_dev; a.capacity = capacity; a.state_floats = (int)fe_resampler_state_floats(rs);
    a.produced = static_cast<int*>(const_cast<void*>(prod_v));
    const bool g711 = resample_is_g711(in_format) || resample_is_g711(out_format);      // (the instantiation that knows the byte formats)
    if constexpr (RING) {
        a.ring_desc = reinterpret_cast<const fe::ResampleRingDesc*>(desc_dev);
        if (g711) rs->last_kernel = pinned ? "fe_resample_kernel<ring,pinned,g711>" : "fe_resample_kernel<ring,g711>";
        else rs->last_kernel = pinned ? "fe_resample_kernel<ring,pinned>" : "fe_resample_kernel<ring>";
        return launch_rc(fe::launch_resample_rings(g711, dim3((unsigned)n), rs->lds_bytes, (hipStream_t)stream, a));
    } else {
        a.desc = reinterpret_cast<const fe::ResampleDesc*>(desc_dev);
        if (g711) rs->last_kernel = pinned ? "fe_resample_kernel<streams,pinned,g711>" : "fe_resample_kernel<streams,g711>";
        else rs->last_kernel = pinned ? "fe_resample_kernel<streams,pinned>" : "fe_resample_kernel<streams>";
        return launch_rc(fe::launch_resample(true, g711, dim3((unsigned)n), rs->lds_bytes, (hipStream_t)stream, a));
    }
}

}  // namespace

extern "C" {

int fe_resampler_create(int sr_in, int sr_out, fe_resampler** out) {
    if (!out) return fail(FE_ERR_INVALID_ARG, "fe_resampler_create: null argument");
    *out = nullptr;
    if (sr_in <= 0 || sr_out <= 0) return fail(FE_ERR_INVALID_ARG, "fe_resampler_create: sample rates must be positive (got %d -> %d)", sr_in, sr_out);
    if (sr_in == sr_out) return fail(FE_ERR_INVALID_ARG, "fe_resampler_create: %d -> %d Hz is no resampling (equal rates)", sr_in, sr_out);
    const long long g = resample_gcd(sr_in, sr_out);
    const long long up = sr_out / g, down = sr_in / g;
    if (up > kResampleMaxRatio || down > kResampleMaxRatio)
        return fail(FE_ERR_UNSUPPORTED_CONFIG, "fe_resampler_create: %d -> %d Hz reduces to the ratio %lld / %lld; the filter is built for max(up, down) <= %d",
                    sr_in, sr_out, up, down, kResampleMaxRatio);
    fe_resampler* rs = new fe_resampler;
    rs->sr_in = sr_in; rs->sr_out = sr_out;
    rs->up = (int)up; rs->down = (int)down;
    const int R = (int)std::max(up, down);
    rs->hl = 10 * R;
    const int L = 2 * rs->hl + 1;
    rs->K = (L + rs->up - 1) / rs->up;
    rs->KP = rs->K | 1;
    // h = up * firwin(L, 1 / R, kaiser 5.0) in double: the windowed sinc scaled to sum 1
    const double pi = 3.14159265358979323846;
    rs->taps.resize((size_t)L);
    double sum = 0.0;
    for (int t = 0; t < L; ++t) {
        const double m = (double)(t - rs->hl);
        const double x = m / (double)R;
        const double sinc = m == 0.0 ? 1.0 : std::sin(pi * x) / (pi * x);
        const double u = m / (double)rs->hl;
        const double w = bessel_i0(5.0 * std::sqrt(std::max(0.0, 1.0 - u * u))) / bessel_i0(5.0);
        rs->taps[(size_t)t] = sinc / (double)R * w;
        sum += rs->taps[(size_t)t];
    }
    for (double& v : rs->taps) v = v / sum * (double)rs->up;
    rs->table.assign((size_t)rs->up * rs->KP, 0.0f);
    for (int r = 0; r < rs->up; ++r)
        for (int j = 0; j < rs->K; ++j)
            if (r + j * rs->up < L) rs->table[(size_t)r * rs->KP + j] = (float)rs->taps[(size_t)(r + j * rs->up)];
    // a tile: at most kResampleTileOut outputs, advancing at most kResampleTileIn input samples; its inputs reach back K - 1 samples
    // (the bound of resample_kernels.hip.h's `span` at r0 = up - 1)
    rs->tile_out = (int)std::min<long long>(kResampleTileOut, std::max<long long>(1, (long long)kResampleTileIn * up / down));
    rs->xcap = (int)((up - 1 + (long long)(rs->tile_out - 1) * down) / up) + rs->K;
    rs->lds_bytes = fe::resample_lds_floats(rs->up, rs->KP, rs->xcap, rs->tile_out) * sizeof(float);
    if (rs->lds_bytes > 160 * 1024) {       // (640 / 1: 51 KB of taps, 67 KB of input - cannot happen below the ratio limit)
        delete rs;
        return fail(FE_ERR_UNSUPPORTED_CONFIG, "fe_resampler_create: %d -> %d Hz needs more than 160 KiB of LDS", sr_in, sr_out);
    }
    *out = rs;
    return FE_OK;
}

void fe_resampler_destroy(fe_resampler* rs) {
    if (!rs) return;
    if (rs->table_dev) (void)hipFree(rs->table_dev);
    delete rs;
}

int fe_resampler_up(const fe_resampler* rs) { return rs ? rs->up : 0; }
int fe_resampler_down(const fe_resampler* rs) { return rs ? rs->down : 0; }
int fe_resampler_taps_per_output(const fe_resampler* rs) { return rs ? rs->K : 0; }
int fe_resampler_half_len(const fe_resampler* rs) { return rs ? rs->hl : 0; }

int fe_resampler_taps(const fe_resampler* rs, double* out, size_t n) {
    if (!rs) return fail(FE_ERR_INVALID_ARG, "fe_resampler_taps: null resampler");
    if (!out) return (int)rs->taps.size();
    if (n < rs->taps.size()) return fail(FE_ERR_INVALID_ARG, "fe_resampler_taps: room for %zu taps, the filter has %zu", n, rs->taps.size());
    std::memcpy(out, rs->taps.data(), rs->taps.size() * sizeof(double));
    return (int)rs->taps.size();
}

long long fe_resampler_out_count(const fe_resampler* rs, long long n_in) {
    if (!rs || n_in < 0) return -1;
    return (n_in * rs->up + rs->down - 1) / rs->down;
}

long long fe_resampler_produced(const fe_resampler* rs, long long consumed, long long n_in) {
    if (!rs || consumed < 0 || n_in < 0) return -1;
    return resample_emitted(rs, consumed + n_in) - resample_emitted(rs, consumed);
}

size_t fe_resampler_state_floats(const fe_resampler* rs) { return rs ? ((size_t)(rs->K - 1) + 2 + 3) / 4 * 4 : 0; }

const char* fe_resampler_last_kernel(const fe_resampler* rs) { return rs ? rs->last_kernel : ""; }

int fe_resample(fe_resampler* rs, const void* in_dev, size_t in_stride, int in_format, long long n_in, void* out_dev, size_t out_stride, int out_format,
                int B, void* stream) {
    const char* fn = "fe_resample";
    if (!rs) return fail(FE_ERR_INVALID_ARG, "%s: null resampler", fn);
    if (!in_dev || !out_dev || B <= 0 || n_in <= 0) return fail(FE_ERR_INVALID_ARG, "%s: bad argument (need non-null pointers, B >= 1, n_in >= 1)", fn);
    int rc = resample_check_format(fn, "in_format", in_format);
    if (rc == FE_OK) rc = resample_check_format(fn, "out_format", out_format);
    if (rc != FE_OK) return rc;
    if (n_in > (1ll << 40)) return fail(FE_ERR_INVALID_ARG, "%s: n_in %lld is more than 2^40 samples", fn, n_in);
    const long long n_out = fe_resampler_out_count(rs, n_in);
    if (in_stride < (size_t)n_in || out_stride < (size_t)n_out)
        return fail(FE_ERR_INVALID_ARG, "%s: strides %zu / %zu are shorter than the rows (%lld samples in, %lld out)", fn, in_stride, out_stride, n_in, n_out);
    const long long tiles = (n_out + rs->tile_out - 1) / rs->tile_out;
    if (B > 65535 || tiles * B > kResampleMaxWorkgroups)
        return fail(FE_ERR_INVALID_ARG, "%s: %lld tiles x %d rows exceed the launch grid (B <= 65535, tiles x B <= %lld: split the call)", fn, tiles, B,
                    kResampleMaxWorkgroups);
    rc = resample_ensure_table(rs, fn);
    if (rc != FE_OK) return rc;
    fe::ResampleArgs a = resample_args(rs, in_dev, in_format, out_dev, out_format);
    a.n_in = n_in; a.n_out = n_out;
    a.in_stride = in_stride; a.out_stride = out_stride;
    const bool g711 = resample_is_g711(in_format) || resample_is_g711(out_format);
    rs->last_kernel = g711 ? "fe_resample_kernel<whole,g711>" : "fe_resample_kernel<whole>";
    return launch_rc(fe::launch_resample(false, g711, dim3((unsigned)tiles, (unsigned)B), rs->lds_bytes, (hipStream_t)stream, a));
}

int fe_resample_streams(fe_resampler* rs, const void* in, size_t in_count, int in_format, float* state_dev, int capacity, const fe_resample_desc* desc_dev,
                        void* out, size_t out_count, int out_format, int* produced, int n, int n_in_max, void* stream) {
    return resample_streams(rs, "fe_resample_streams", false, in, in_count, in_format, state_dev, capacity, desc_dev, out, out_count, out_format, produced, n,
                            n_in_max, stream);
}

int fe_resample_streams_pinned(fe_resampler* rs, const void* in, size_t in_count, int in_format, float* state_dev, int capacity,
                               const fe_resample_desc* desc_dev, void* out, size_t out_count, int out_format, int* produced, int n, int n_in_max,
                               void* stream) {
    return resample_streams(rs, "fe_resample_streams_pinned", true, in, in_count, in_format, state_dev, capacity, desc_dev, out, out_count, out_format,
                            produced, n, n_in_max, stream);
}

int fe_resample_rings(fe_resampler* rs, const void* in, size_t in_count, int in_format, float* state_dev, int capacity,
                      const fe_resample_ring_desc* desc_dev, void* out, size_t out_count, int out_format, int* produced, int n, int n_in_max,
                      void* stream) {
    return resample_streams(rs, "fe_resample_rings", false, in, in_count, in_format, state_dev, capacity, desc_dev, out, out_count, out_format, produced, n,
                            n_in_max, stream);
}

int fe_resample_rings_pinned(fe_resampler* rs, const void* in, size_t in_count, int in_format, float* state_dev, int capacity,
                             const fe_resample_ring_desc* desc_dev, void* out, size_t out_count, int out_format, int* produced, int n, int n_in_max,
                             void* stream) {
    return resample_streams(rs, "fe_resample_rings_pinned", true, in, in_count, in_format, state_dev, capacity, desc_dev, out, out_count, out_format,
                            produced, n, n_in_max, stream);
}

}  // extern "C"
