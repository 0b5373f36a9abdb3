// fe_api_fspen.inc - host side of FSPEN: weight sections, handle creation, packer, launch (included by fe_api.hip inside its anonymous namespace)
// ============================================================================ FSPEN (models/fspen/model.py)
// fused state_dict of ONNXModel after remove_weight_reparameterizations (:299-340), reference layouts
const int kSeK[5] = {4, 7, 11, 20, 40};                   // SubbandEncoder kernels (:41-44)
const int kSdN[5] = {2, 3, 5, 10, 20};                    // SubbandDecoder outputs per row (:70)

// The family as fe_api.hip's shared baseline-family paths see it (visit_baseline: the stream and spec steps, offline, the buffer sizes, debug stages)
struct FspenFamily {
    using Args = fe::FArgs;
    using StreamArgs = fe::FStreamArgs;
    static const fe::FImpl* impl(const fe_handle* h) { return h->fimpl; }
    static const char* shape_name(const fe_handle*) { return "fspen"; }
    static float*& state(Args& a) { return a.gru; }
    static size_t state_floats(const fe_handle*, int B) { return (size_t)B * fe::FShape<256>::CACHE_FLOATS; }
    // the model's state of `cap` streams as regions from float `off` on (state_regions): the inter-GRU states [NB * G][cap][F / G][C]
    static int regions(const fe_handle*, size_t, size_t off, StateRegion* r) {
        using S = fe::FShape<256>;
        r[0] = {off, S::NCACHE, S::FG * S::C};
        return 1;
    }
    static size_t counters(const fe_handle* h) { return h->fimpl->num_blocks; }      // time-pipeline frame counters per stream
    static constexpr int kPipeFrames = 32;
    static constexpr bool kPipeCarriesState = true;      // (fe_step_backlog: the PIPE kernel's frames hand the streaming state on in place)
    static constexpr bool kPipeCarriesStateOnRequest = false;      // (it always does: nothing to ask for)
    static size_t ring_floats(const fe_handle*) { return 0; }
    static void set_ring(Args&, float*) {}
    static size_t xp_floats(const fe_handle*) { return 0; }
    static StreamArgs args(fe_handle* h, int B, int T);
    static int create(const fe_config* cfg, fe_handle** out);
    static int pack_weights(fe_handle* h, const Blob& S, std::vector<float>* out);
    static int ensure_sb(fe_handle* h, int B);
    static int launch_step(fe_handle* h, StreamArgs& a, fe::StepFlavour flavour, void* stream);
    static const char* stage_name(const fe_handle*, int idx);
    static double macs(const fe_handle* h);
};

void build_sections_fspen(fe_handle* h) {
    char nm[160];
    for (int i = 0; i < 5; ++i) {
        snprintf(nm, sizeof nm, "subband_encoder.conv%d.0.weight", i + 1); add_section(h, nm, {32, 1, kSeK[i]});
        snprintf(nm, sizeof nm, "subband_encoder.conv%d.0.bias", i + 1); add_section(h, nm, {32});
    }
    for (int i = 0; i < 5; ++i) {
        snprintf(nm, sizeof nm, "subband_decoder.lin%d.0.weight", i + 1); add_section(h, nm, {kSdN[i], 64});
        snprintf(nm, sizeof nm, "subband_decoder.lin%d.0.bias", i + 1); add_section(h, nm, {kSdN[i]});
    }
    const int C1[3] = {4, 16, 32}, K[3] = {6, 8, 6};
    for (int i = 0; i < 3; ++i) {
        snprintf(nm, sizeof nm, "fullband_encoder.%d.0.weight", i); add_section(h, nm, {C1[i], i == 0 ? 2 : C1[i - 1], K[i]});
        snprintf(nm, sizeof nm, "fullband_encoder.%d.0.bias", i); add_section(h, nm, {C1[i]});
    }
    add_section(h, "fullband_encoder_post.weight", {32, 32, 1});
    add_section(h, "feature_merge.0.weight", {32, 64});
    add_section(h, "feature_merge.2.weight", {16, 32, 1});
    add_section(h, "feature_merge.2.bias", {16});
    for (int b = 0; b < 3; ++b) {
        auto gru = [&](const std::string& p, const char* sfx) {
            add_section(h, p + ".weight_ih_l0" + sfx, {48, 16});
            add_section(h, p + ".weight_hh_l0" + sfx, {48, 16});
            add_section(h, p + ".bias_ih_l0" + sfx, {48});
            add_section(h, p + ".bias_hh_l0" + sfx, {48});
        };
        snprintf(nm, sizeof nm, "dpe_blocks.%d.", b);
        const std::string p = nm;
        gru(p + "intra_rnn", "");
        gru(p + "intra_rnn", "_reverse");
        add_section(h, p + "intra_fc.weight", {16, 32});
        add_section(h, p + "intra_fc.bias", {16});
        add_section(h, p + "intra_ln.weight", {32, 16});
        add_section(h, p + "intra_ln.bias", {32, 16});
        for (int g = 0; g < 8; ++g) gru(p + "inter_rnn.inter_rnn." + std::to_string(g), "");
        for (int g = 0; g < 8; ++g) {
            add_section(h, p + "inter_rnn.inter_fc." + std::to_string(g) + ".weight", {16, 16});
            add_section(h, p + "inter_rnn.inter_fc." + std::to_string(g) + ".bias", {16});
        }
    }
    add_section(h, "feature_split.0.weight", {32, 16, 1});
    add_section(h, "feature_split.0.bias", {32});
    add_section(h, "feature_split.1.weight", {64, 32});
    for (int j = 0; j < 3; ++j) {
        const int i = 2 - j, cin = C1[i], cout = i == 0 ? 2 : C1[i - 1];
        snprintf(nm, sizeof nm, "fullband_decoder.%d.0.weight", j); add_section(h, nm, {cin, 2 * cin, 1});
        snprintf(nm, sizeof nm, "fullband_decoder.%d.1.weight", j); add_section(h, nm, {cin, cout, K[i]});
        snprintf(nm, sizeof nm, "fullband_decoder.%d.1.bias", j); add_section(h, nm, {cout});
    }
}

int FspenFamily::create(const fe_config* cfg, fe_handle** out) {
    if (cfg->n_fft != 512) return fail(FE_ERR_INVALID_ARG, "Only n_fft == 512 is allowed, but given %d", cfg->n_fft);
    if (cfg->win_size > cfg->n_fft) return fail(FE_ERR_INVALID_ARG, "n_fft(%d) must be bigger than win_size(%d)", cfg->n_fft, cfg->win_size);
    // the one architecture of configs/others/fspen.yaml: channels [4, 16, 32], kernel_size [6, 8, 6], stride 2, DPE 3 x (16 ch, 32 bands, 8 groups)
    const bool ok = cfg->channels == 32 && cfg->n_kernels == 3 && cfg->kernel_size[0] == 6 && cfg->kernel_size[1] == 8 && cfg->kernel_size[2] == 6 &&
                    cfg->stride == 2 && cfg->rf_channels == 16 && cfg->rf_freq == 32 && cfg->rf_blocks == 3 && cfg->rf_heads == 8;
    const fe::FImpl* fi = (ok && cfg->hop_size == 256) ? fe_fimpl_h256() : nullptr;
    if (!fi)
        return fail(FE_ERR_UNSUPPORTED_CONFIG, "no FSPEN kernel compiled for channels[-1]=%d kernels=%d dpe=(%d blocks, %d ch, %d bands, %d groups) hop=%d "
                    "(configs/others/fspen.yaml is the compiled architecture)", cfg->channels, cfg->n_kernels, cfg->rf_blocks, cfg->rf_channels,
                    cfg->rf_freq, cfg->rf_heads, cfg->hop_size);
    fe_handle* h = new_handle(cfg, Dims{32, 0, 16, 32, 3, cfg->n_fft, cfg->hop_size, cfg->n_fft / 2, 0, 0, {0}});
    h->fimpl = fi;
    build_sections_fspen(h);
    *out = h;
    return FE_OK;
}

// k-major repack of the fused weights at the compile-time offsets of fe::FPk (fspen_kernels.hip.h)
int FspenFamily::pack_weights(fe_handle* h, const Blob& S, std::vector<float>* out) {
    using P = fe::FPk;
    fe::frag::Buffer buf(P::TOTAL);
    char nm[160];
    pack_stft_tables(buf, h, P::WINDOW, P::WINDOW_I, P::TW);
    for (int i = 0, row = 0; i < 5; row += kSeK[i], ++i) {
        snprintf(nm, sizeof nm, "subband_encoder.conv%d.0.weight", i + 1);
        const float* w = S(nm);                                       // (32, 1, K)
        snprintf(nm, sizeof nm, "subband_encoder.conv%d.0.bias", i + 1);
        const float* b = S(nm);
        for (int ch = 0; ch < 32; ++ch) {
            for (int k = 0; k < kSeK[i]; ++k) buf[P::SE_W + (row + k) * 32 + ch] = w[ch * kSeK[i] + k];
            buf[P::SE_B + i * 32 + ch] = b[ch];
        }
    }
    // Conv1d (Cout, Cin, K) -> [(c*K + k)][Cout]
    auto conv = [&](const char* key, int cout, int cin, int K, int dst_w, int dst_b) {
        const float* w = S(std::string(key) + ".weight");
        for (int o = 0; o < cout; ++o)
            for (int c = 0; c < cin; ++c)
                for (int k = 0; k < K; ++k) buf[dst_w + (c * K + k) * cout + o] = w[(o * cin + c) * K + k];
        if (dst_b >= 0) { const float* b = S(std::string(key) + ".bias"); for (int o = 0; o < cout; ++o) buf[dst_b + o] = b[o]; }
    };
    conv("fullband_encoder.0.0", 4, 2, 6, P::FE0_W, P::FE0_B);
    conv("fullband_encoder.1.0", 16, 4, 8, P::FE1_W, P::FE1_B);
    conv("fullband_encoder.2.0", 32, 16, 6, P::FE2_W, P::FE2_B);
    conv("fullband_encoder_post", 32, 32, 1, P::POST_W, -1);
    {   // feature_merge.0 Linear (32 out j, 64 in i) -> [i][j]
        const float* w = S("feature_merge.0.weight");
        for (int j = 0; j < 32; ++j) for (int i = 0; i < 64; ++i) buf[P::MG1_W + i * 32 + j] = w[j * 64 + i];
    }
    conv("feature_merge.2", 16, 32, 1, P::MG2_W, P::MG2_B);
    // GRU (gate order r, z, n): W_ih^T [k][48]; bias = b_ih + (b_hh for r, z); b_hh of n kept apart (it sits inside r * (...))
    auto gru_ih = [&](const std::string& p, const char* sfx, int dst_w, int dst_gb, int dst_hn) {
        const float* wi = S(p + ".weight_ih_l0" + sfx);
        const float* bi = S(p + ".bias_ih_l0" + sfx);
        const float* bh = S(p + ".bias_hh_l0" + sfx);
        for (int g = 0; g < 48; ++g) {
            for (int k = 0; k < 16; ++k) buf[dst_w + k * 48 + g] = wi[g * 16 + k];
            buf[dst_gb + g] = bi[g] + (g < 32 ? bh[g] : 0.0f);
        }
        for (int c = 0; c < 16; ++c) buf[dst_hn + c] = bh[32 + c];
    };
    for (int b = 0; b < 3; ++b) {
        const int D = P::DPE + b * P::D_SIZE;
        snprintf(nm, sizeof nm, "dpe_blocks.%d.", b);
        const std::string p = nm;
        for (int d = 0; d < 2; ++d) {
            const char* sfx = d ? "_reverse" : "";
            gru_ih(p + "intra_rnn", sfx, D + P::D_IH + d * 768, D + P::D_GB + d * 48, D + P::D_HN + d * 16);
            const float* wh = S(p + "intra_rnn.weight_hh_l0" + sfx);       // (48, 16) -> [gate][k][unit]
            for (int gate = 0; gate < 3; ++gate)
                for (int k = 0; k < 16; ++k)
                    for (int c = 0; c < 16; ++c) buf[D + P::D_HH + ((d * 3 + gate) * 16 + k) * 16 + c] = wh[(gate * 16 + c) * 16 + k];
        }
        {
            const float* w = S(p + "intra_fc.weight");                      // (16, 32) -> [k][c]
            const float* bb = S(p + "intra_fc.bias");
            for (int c = 0; c < 16; ++c) { for (int k = 0; k < 32; ++k) buf[D + P::D_FC_W + k * 16 + c] = w[c * 32 + k]; buf[D + P::D_FC_B + c] = bb[c]; }
            const float* lw = S(p + "intra_ln.weight");
            const float* lb = S(p + "intra_ln.bias");
            for (int i = 0; i < 512; ++i) { buf[D + P::D_LN_W + i] = lw[i]; buf[D + P::D_LN_B + i] = lb[i]; }
        }
        for (int g = 0; g < 8; ++g) {
            const int Gb = D + P::D_G + g * P::G_SIZE;
            const std::string q = p + "inter_rnn.inter_rnn." + std::to_string(g);
            gru_ih(q, "", Gb + P::G_IH, Gb + P::G_GB, Gb + P::G_HN);
            const float* wh = S(q + ".weight_hh_l0");
            for (int gg = 0; gg < 48; ++gg) for (int k = 0; k < 16; ++k) buf[Gb + P::G_HH + k * 48 + gg] = wh[gg * 16 + k];
            const float* fw = S(p + "inter_rnn.inter_fc." + std::to_string(g) + ".weight");
            const float* fb = S(p + "inter_rnn.inter_fc." + std::to_string(g) + ".bias");
            for (int c = 0; c < 16; ++c) { for (int k = 0; k < 16; ++k) buf[Gb + P::G_FC_W + k * 16 + c] = fw[c * 16 + k]; buf[Gb + P::G_FC_B + c] = fb[c]; }
        }
    }
    {   // stream-batched DPE (fspen_sb_kernels.hip.h): A-operand fragments (fe_fragments.h, plain order) and the tiles' per-row biases;
        // the r / z rows and biases carry -log2 e, the n rows 2 log2 e (sigma / tanh as one exp2 + rcp of the pre-scaled value)
        using Q = fe::FSbPk;
        const float kRZ = -1.4426950408889634f, kN = 2.8853900817779268f;
        auto feat = [](int row) { return 4 * (row & 3) + (row >> 2); };        // output row 4 lg + r  <->  feature 4 r + lg
        // GRU bias of (unit u, gate g of r, z, n_x, n_h)
        auto gbias = [&](const float* bi, const float* bh, int u, int g) {
            return g == 0 ? (bi[u] + bh[u]) * kRZ : g == 1 ? (bi[16 + u] + bh[16 + u]) * kRZ : g == 2 ? bi[32 + u] * kN : bh[32 + u] * kN;
        };
        for (int b = 0; b < 3; ++b) {
            const int D = P::SB + b * Q::D_SIZE;
            snprintf(nm, sizeof nm, "dpe_blocks.%d.", b);
            const std::string p = nm;
            for (int d = 0; d < 2; ++d) {
                const char* sfx = d ? "_reverse" : "";
                const float* wi = S(p + "intra_rnn.weight_ih_l0" + sfx);      // (48, 16), gate order r, z, n
                const float* wh = S(p + "intra_rnn.weight_hh_l0" + sfx);
                const float* bi = S(p + "intra_rnn.bias_ih_l0" + sfx);
                const float* bh = S(p + "intra_rnn.bias_hh_l0" + sfx);
                for (int q = 0; q < 4; ++q) {
                    const int wave = d * 4 + q;
                    // row 4 j + g = (unit u = 4 q + j, gate g of r, z, n_x, n_h): k < 16 the x half (n_h: zero), k >= 16 the h half (n_x: zero)
                    buf.tiles(D + Q::I_W + wave * 8 * 64, 1, 8, [&](int, int row, int k) {
                        const int u = 4 * q + (row >> 2), g = row & 3;
                        if (g == (k < 16 ? 3 : 2)) return 0.0f;
                        return (k < 16 ? wi : wh)[((g < 2 ? g : 2) * 16 + u) * 16 + k % 16] * (g < 2 ? kRZ : kN);
                    });
                    buf.rows(D + Q::I_B + wave * 16, 1, [&](int, int row) { return gbias(bi, bh, 4 * q + (row >> 2), row & 3); });
                }
            }
            {
                const float* w = S(p + "intra_fc.weight");                      // (16, 32)
                const float* bb = S(p + "intra_fc.bias");
                const float* lw = S(p + "intra_ln.weight");
                const float* lb = S(p + "intra_ln.bias");
                buf.tiles(D + Q::FC_W, 1, 8, [&](int, int row, int k) { return w[feat(row) * 32 + k]; });
                buf.rows(D + Q::FC_B, 1, [&](int, int row) { return bb[feat(row)]; });
                buf.rows(D + Q::LN_W, 32, [&](int f, int row) { return lw[f * 16 + feat(row)]; });
                buf.rows(D + Q::LN_B, 32, [&](int f, int row) { return lb[f * 16 + feat(row)]; });
            }
            for (int g = 0; g < 8; ++g) {
                const int Gb = D + Q::GRP + g * Q::G_SIZE;
                const std::string q = p + "inter_rnn.inter_rnn." + std::to_string(g);
                const float* wi = S(q + ".weight_ih_l0");
                const float* wh = S(q + ".weight_hh_l0");
                const float* bi = S(q + ".bias_ih_l0");
                const float* bh = S(q + ".bias_hh_l0");
                const float* fw = S(p + "inter_rnn.inter_fc." + std::to_string(g) + ".weight");
                const float* fb = S(p + "inter_rnn.inter_fc." + std::to_string(g) + ".bias");
                // 24 k-steps: r (x | h), z (x | h), n_x, n_h
                buf.tiles(Gb + Q::G_W, 1, 24, [&](int, int row, int k) {
                    const int i = k / 4, gate = i < 8 ? 0 : (i < 16 ? 1 : 2), ksl = i < 16 ? (i & 7) : i - 16;      // ksl < 4: x half, else h half
                    return (ksl < 4 ? wi : wh)[(gate * 16 + feat(row)) * 16 + 4 * (ksl & 3) + k % 4] * (gate < 2 ? kRZ : kN);
                });
                buf.rows(Gb + Q::G_B, 4, [&](int gt, int row) { return gbias(bi, bh, feat(row), gt); });
                buf.rows(Gb + Q::G_FCB, 1, [&](int, int row) { return fb[feat(row)]; });
                buf.tiles(Gb + Q::G_FCW, 1, 4, [&](int, int row, int k) { return fw[feat(row) * 16 + k]; });
            }
        }
        // stream-batched fullband_encoder_post, feature merge / split, fullband_decoder.0's 1x1 (fspen_sb_kernels.hip.h)
        const float* wpo = S("fullband_encoder_post.weight");  // (32, 32, 1)
        const float* wf2 = S("fullband_encoder.2.0.weight");   // Conv1d (32, 16, 6)
        const float* bf2 = S("fullband_encoder.2.0.bias");
        const float* w1 = S("feature_merge.0.weight");        // (32, 64)
        const float* w2 = S("feature_merge.2.weight");        // (16, 32, 1)
        const float* b2 = S("feature_merge.2.bias");
        const float* s1 = S("feature_split.0.weight");        // (32, 16, 1)
        const float* sb1 = S("feature_split.0.bias");
        const float* s2 = S("feature_split.1.weight");        // (64, 32)
        const float* wd0 = S("fullband_decoder.0.0.weight");  // (32, 64, 1)
        const float* wd1 = S("fullband_decoder.1.0.weight");  // (16, 32, 1)
        const float* wd1t = S("fullband_decoder.1.1.weight"); // ConvTranspose1d (16 in, 4 out, 8)
        const float* bd1t = S("fullband_decoder.1.1.bias");
        const float* wdt = S("fullband_decoder.0.1.weight");  // ConvTranspose1d (32 in, 16 out, 6)
        const int SB = P::SB;
        buf.rows(SB + Q::FD1T_B, 1, [&](int, int row) { return row < 8 ? bd1t[row & 3] : 0.0f; });
        buf.raw(SB + Q::FD0T_B, 16, S("fullband_decoder.0.1.bias"));
        buf.tiles(SB + Q::FE2_W, 2, 24, [&](int ot, int row, int k) { return wf2[((16 * ot + feat(row)) * 16 + k % 16) * 6 + k / 16]; });      // k = tap * 16 + channel
        buf.tiles(SB + Q::POST_W, 2, 8, [&](int ot, int row, int k) { return wpo[(16 * ot + feat(row)) * 32 + k]; });
        buf.tiles(SB + Q::MG1_W, 2, 16, [&](int jt, int row, int k) {
            const int ks = k / 4, lg = k % 4, i = ks < 8 ? k : 32 + 16 * ((ks - 8) >> 2) + 4 * lg + ((ks - 8) & 3);
            return w1[(16 * jt + feat(row)) * 64 + i];
        });
        buf.tiles(SB + Q::MG2_W, 1, 8, [&](int, int row, int k) { return w2[feat(row) * 32 + k]; });
        buf.tiles(SB + Q::SP1_W, 2, 4, [&](int ct, int row, int k) { return s1[(16 * ct + feat(row)) * 16 + k]; });
        buf.tiles(SB + Q::SP2_W, 4, 8, [&](int jt, int row, int k) { return s2[(16 * jt + (jt < 2 ? feat(row) : row)) * 32 + k]; });
        // (rows 4 lg + r <-> output 4 r + lg: its output is the next product's B operand, stored to LDS)
        buf.tiles(SB + Q::FD0_W, 2, 16, [&](int ot, int row, int k) { return wd0[(16 * ot + feat(row)) * 64 + k]; });
        buf.tiles(SB + Q::FD0T_W, 6, 8, [&](int t, int row, int k) { return wdt[(k * 16 + row) * 6 + t / 3 + 2 * (t % 3)]; });      // tile = parity * 3 + tap pair
        buf.tiles(SB + Q::FD1_W, 1, 8, [&](int, int row, int k) { const int ks = k / 4, lg = k % 4; return wd1[feat(row) * 32 + (ks < 4 ? 4 * lg + ks : 16 + 4 * (ks - 4) + lg)]; });
        buf.tiles(SB + Q::FD1T_W, 5, 4, [&](int j, int row, int k) {
            const int par = row >> 2, o = row & 3, tap = (par ? 8 : 7) - 2 * j;      // output positions 2 m + par <- input position m - 2 + j
            return (row < 8 && tap >= 0 && tap < 8) ? wd1t[(k * 4 + o) * 8 + tap] : 0.0f;
        });
        buf.rows(SB + Q::MG2_B, 1, [&](int, int row) { return b2[feat(row)]; });
        buf.rows(SB + Q::FE2_B, 2, [&](int ot, int row) { return bf2[16 * ot + feat(row)]; });
        buf.rows(SB + Q::SP1_B, 2, [&](int ct, int row) { return sb1[16 * ct + feat(row)]; });
    }
    conv("feature_split.0", 32, 16, 1, P::SP1_W, P::SP1_B);
    {   // feature_split.1 Linear (64 out j, 32 in f) -> [f][j]
        const float* w = S("feature_split.1.weight");
        for (int j = 0; j < 64; ++j) for (int f = 0; f < 32; ++f) buf[P::SP2_W + f * 64 + j] = w[j * 32 + f];
    }
    {   // sub-band decoder (SubbandDecoder.forward, :83-95): bin -> (layer, output o of its row): one weight column per bin
        const int base[5] = {0, 16, 32, 64, 128}, k0[5] = {0, 1, 4, 8, 16}, keep[5] = {16, 16, 32, 64, 129};
        for (int i = 0; i < 5; ++i) {
            snprintf(nm, sizeof nm, "subband_decoder.lin%d.0.weight", i + 1);
            const float* w = S(nm);                                   // (n, 64)
            snprintf(nm, sizeof nm, "subband_decoder.lin%d.0.bias", i + 1);
            const float* bb = S(nm);
            for (int q = 0; q < keep[i]; ++q) {
                const int bin = base[i] + q, o = (k0[i] + q) % kSdN[i];
                for (int k = 0; k < 64; ++k) buf[P::SD_W + ((k / 4) * 260 + bin) * 4 + k % 4] = w[o * 64 + k];
                buf[P::SD_B + bin] = bb[o];
            }
        }
    }
    // ConvTranspose1d (Cin, Cout, K) -> [(c*K + k)][Cout]
    auto convt = [&](const char* key, int cin, int cout, int K, int dst_w, int dst_b) {
        const float* w = S(std::string(key) + ".weight");
        const float* b = S(std::string(key) + ".bias");
        for (int c = 0; c < cin; ++c)
            for (int o = 0; o < cout; ++o)
                for (int k = 0; k < K; ++k) buf[dst_w + (c * K + k) * cout + o] = w[(c * cout + o) * K + k];
        for (int o = 0; o < cout; ++o) buf[dst_b + o] = b[o];
    };
    conv("fullband_decoder.0.0", 32, 64, 1, P::FD0_W, -1);
    convt("fullband_decoder.0.1", 32, 16, 6, P::FD0_T, P::FD0_B);
    conv("fullband_decoder.1.0", 16, 32, 1, P::FD1_W, -1);
    convt("fullband_decoder.1.1", 16, 4, 8, P::FD1_T, P::FD1_B);
    conv("fullband_decoder.2.0", 4, 8, 1, P::FD2_W, -1);
    convt("fullband_decoder.2.1", 4, 2, 6, P::FD2_T, P::FD2_B);
    *out = std::move(buf.v);
    return FE_OK;
}

fe::FStreamArgs FspenFamily::args(fe_handle* h, int B, int T) {
    fe::FStreamArgs a{};
    a.wp = h->packed_dev;
    a.B = B;
    a.T = T;
    a.compression = h->cfg.input_compression;
    return a;
}

// FSPEN per-hop step of large batches: the middle of the network batched over the streams (fspen_sb_kernels.hip.h) from FE_FSPEN_SB streams
// (0 = never; measured crossover on 256 CUs at ~1500 streams - a sixteen-stream workgroup per CU needs 4096 to fill the chip)
// (fe_set_option("fspen_stream_batch_min", n); default 1536)
int FspenFamily::ensure_sb(fe_handle* h, int B) {
    // (+ 16: the last stream tile's lane-private scratch is whole)
    return ensure_sb_scratch(h, B, h->opt[OPT_FSPEN_SB_MIN], ((size_t)B + 16) * h->fimpl->split_floats_per_stream * sizeof(float));
}

// Every launch of the per-stream kernel.  The plain flavour may grow the stream-batched scratch and run the per-hop step of a large batch through
// it; the slotted and packet flavours (fe_step_pool, fe_step_pool_streams[_pinned]) run the per-stream kernel in their own instantiation at every
// batch size (the stream-batched middle's tensors are laid out per call tile) and allocate nothing.
int FspenFamily::launch_step(fe_handle* h, fe::FStreamArgs& a, fe::StepFlavour flavour, void* stream) {
    hipError_t e = hipSuccess;
    const int sb_min = h->opt[OPT_FSPEN_SB_MIN];
    if (flavour == fe::STEP_PLAIN && a.mode == fe::FE_MODE_STREAM && a.T == 1 && a.dbg == nullptr && sb_min > 0 && a.B >= sb_min) {      // (fe_profile_step: the DPE kernel's counters only)
        const int rc = ensure_sb(h, a.B);
        if (rc != FE_OK) return rc;
        a.tok = h->sb_dev;
        a.carry = a.tok + (size_t)a.B * 2048;
        h->fimpl->launch_sb(a, h->max_wgs, (hipStream_t)stream, &e);
        return launch_rc(e);
    }
    h->fimpl->launch_step(a, flavour, h->max_wgs, (hipStream_t)stream, &e);
    return launch_rc(e);
}

const char* FspenFamily::stage_name(const fe_handle*, int idx) {
    static const char* const names[16] = {"spec_in", "compressed", "subband_encoder", "fullband_encoder.2", "feature_merge", "dpe.0.intra",
                                          "dpe.0.inter", "dpe.1.intra", "dpe.1.inter", "dpe.2.intra", "dpe.2.inter", "feature_split",
                                          "fullband_decoder.0", "fullband_decoder.1", "mask", "spec_out"};
    return names[idx];
}

double FspenFamily::macs(const fe_handle*) {   // models/fspen/macs.py:36-141 with T = 1 (switches as committed: conv output lengths, no BN / LN / bias terms)
    const double C1[3] = {4, 16, 32}, K[3] = {6, 8, 6}, C2 = 16;
    double F = 257, m = 0;
    for (int i = 0; i < 3; ++i) { F = std::floor(F / 2); m += (i == 0 ? 2 : C1[i - 1]) * C1[i] * F * K[i]; }
    m += 32 * 32 * F + 32 * (4 * 8 + 7 * 6 + 11 * 6 + 20 * 6 + 40 * 6) + 32 * 64 * 32 + 32 * C2 * 32;
    const double gru = (C2 + C2) * C2 * 3 + C2 * 3;
    m += 3 * (gru * 2 + 2 * C2 * C2 + C2 + gru + C2 * C2 + C2) * 32;
    m += C2 * 32 * 32 + 32 * 32 * 64 + 32 * (8 * 2 + 6 * 3 + 8 * 5 + 8 * 10 + 8 * 20);
    for (int i = 2; i >= 0; --i) { m += C1[i] * (i == 0 ? 2 : C1[i - 1]) * F * K[i]; F = i == 0 ? F * 2 + 1 : F * 2; }
    m += 257 * 8;
    return m;
}
