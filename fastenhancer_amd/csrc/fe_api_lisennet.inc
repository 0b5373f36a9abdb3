// fe_api_lisennet.inc - host side of LiSenNet: weight sections, handle creation, packer, launch (included by fe_api.hip inside its anonymous namespace)
// ============================================================================ LiSenNet (models/lisennet/model.py)

// The family as fe_api.hip's shared baseline-family paths see it (visit_baseline: the stream and spec steps, offline, the buffer sizes, debug stages)
struct LisennetFamily {
    using Args = fe::LArgs;
    using StreamArgs = fe::LStreamArgs;
    static const fe::LImpl* impl(const fe_handle* h) { return h->limpl; }
    static const char* shape_name(const fe_handle*) { return "lisennet"; }
    static float*& state(Args& a) { return a.cache; }
    static size_t state_floats(const fe_handle* h, int B) { return (size_t)B * h->limpl->cache_floats; }
    // the model's state of `cap` streams as regions from float `off` on (state_regions): the nine caches in the order of the reference's
    // list, each [cap][its floats per stream]
    static int regions(const fe_handle*, size_t cap, size_t off, StateRegion* r) {
        using S = fe::LShape<256>;
        int n = 0;
        auto add = [&](int len) { r[n++] = {off, 1, len}; off += cap * (size_t)len; };
        add(S::K_PHA); add(S::K_E2); add(S::K_E3); add(S::K_E4);
        for (int b = 0; b < S::NB; ++b) { add(S::K_H); add(S::K_GLU); }
        add(S::K_DEC);
        return n;
    }
    static size_t counters(const fe_handle* h) { return h->limpl->nsite; }      // time-pipeline frame counters per stream
    static constexpr int kPipeFrames = 32;
    // fe_step_backlog walks unless it is asked not to: the PIPE kernel hands the nine caches through ring slots and starts from zero caches at
    // frame 0 (cprev / ccur in lisennet_kernels.hip.h).  Its CARRY instantiation takes frame 0's caches from the caller's state and leaves the
    // last frames' there, in place - under an explicit fe_set_time_pipeline(P >= 2) and with a work buffer of
    // fe_lisennet_backlog_work_floats (which has the ring; fe_step_backlog_work_floats stays 0), fe_step_backlog launches that one.
    // fe_step_pool_streams_chunk, on the same terms and with fe_lisennet_pool_streams_chunk_work_floats: its packet form (LImpl::launch_streams_pipe).
    static constexpr bool kPipeCarriesState = false;
    static constexpr bool kPipeCarriesStateOnRequest = true;
    static void launch_pipe_stream(const fe_handle* h, const Args& a, hipStream_t st, hipError_t* e) { h->limpl->launch_pipe_stream(a, st, e); }
    // the time pipeline's ring of the caches of the frames in flight (LArgs::ring), sized for the widest pipeline: two more slots than frames
    static size_t ring_floats(const fe_handle* h) { return (size_t)(kMaxPipeFrames + 2) * h->limpl->cache_floats; }
    static void set_ring(Args& a, float* ring) { a.ring = ring; }
    static size_t xp_floats(const fe_handle*) { return 0; }
    static StreamArgs args(fe_handle* h, int B, int T);
    static int create(const fe_config* cfg, fe_handle** out);
    static int pack_weights(fe_handle* h, const Blob& S, std::vector<float>* out);
    static int ensure_sb(fe_handle* h, int B);
    static int launch_step(fe_handle* h, StreamArgs& a, fe::StepFlavour flavour, void* stream);
    static const char* stage_name(const fe_handle*, int idx);
    static double macs(const fe_handle* h);
};

// the checkpoint as it is (remove_weight_reparameterizations is a no-op, :476-477), reference layouts, module order
void build_sections_lisennet(fe_handle* h) {
    const int C = 16, c1 = 4, c2 = 8, c3 = 12, F = 257, Hd = 24, nf = 32;
    auto dsconv = [&](const std::string& p, int cin, int cout, int nfq) {
        add_section(h, p + ".low_conv.weight", {cout, cin, 2, 3});
        add_section(h, p + ".low_conv.bias", {cout});
        add_section(h, p + ".high_conv.weight", {cout, cin, 2, 5});
        add_section(h, p + ".high_conv.bias", {cout});
        add_section(h, p + ".norm.gamma", {1, 1, 1, nfq / 2});
        add_section(h, p + ".norm.beta", {1, 1, 1, nfq / 2});
        add_section(h, p + ".act.weight", {cout});
    };
    auto gru = [&](const std::string& p, int i, int hd, bool bi) {
        for (const char* sfx : {"", "_reverse"}) {
            if (!bi && sfx[0]) break;
            add_section(h, p + ".weight_ih_l0" + sfx, {3 * hd, i});
            add_section(h, p + ".weight_hh_l0" + sfx, {3 * hd, hd});
            add_section(h, p + ".bias_ih_l0" + sfx, {3 * hd});
            add_section(h, p + ".bias_hh_l0" + sfx, {3 * hd});
        }
    };
    add_section(h, "encoder.conv_1.0.weight", {c1, 3, 1, 1});
    add_section(h, "encoder.conv_1.0.bias", {c1});
    add_section(h, "encoder.conv_1.1.gamma", {1, 1, 1, F});
    add_section(h, "encoder.conv_1.1.beta", {1, 1, 1, F});
    add_section(h, "encoder.conv_1.2.weight", {c1});
    dsconv("encoder.conv_2", c1, c2, F);
    dsconv("encoder.conv_3", c2, c3, F / 2);
    dsconv("encoder.conv_4", c3, C, F / 4);
    for (int b = 0; b < 2; ++b) {
        const std::string p = "blocks." + std::to_string(b) + ".";
        add_section(h, p + "dp_rnn_attn.intra_norm.weight", {nf, C});
        add_section(h, p + "dp_rnn_attn.intra_norm.bias", {nf, C});
        gru(p + "dp_rnn_attn.intra_rnn_attn.rnn", C, Hd / 2, true);
        add_section(h, p + "dp_rnn_attn.intra_rnn_attn.dense.weight", {C, Hd});
        add_section(h, p + "dp_rnn_attn.intra_rnn_attn.dense.bias", {C});
        add_section(h, p + "dp_rnn_attn.inter_norm.weight", {nf, C});
        add_section(h, p + "dp_rnn_attn.inter_norm.bias", {nf, C});
        gru(p + "dp_rnn_attn.inter_rnn_attn.rnn", C, Hd, false);
        add_section(h, p + "dp_rnn_attn.inter_rnn_attn.dense.weight", {C, Hd});
        add_section(h, p + "dp_rnn_attn.inter_rnn_attn.dense.bias", {C});
        add_section(h, p + "conv_glu.norm.gamma", {1, C, 1, nf});
        add_section(h, p + "conv_glu.norm.beta", {1, C, 1, nf});
        add_section(h, p + "conv_glu.fc1.weight", {4 * C, C, 1, 1});
        add_section(h, p + "conv_glu.fc1.bias", {4 * C});
        add_section(h, p + "conv_glu.dwconv.weight", {2 * C, 1, 3, 3});
        add_section(h, p + "conv_glu.dwconv.bias", {2 * C});
        add_section(h, p + "conv_glu.fc2.weight", {C, 2 * C, 1, 1});
        add_section(h, p + "conv_glu.fc2.bias", {C});
    }
    const int ucin[3] = {2 * C, 2 * c3, 2 * c2}, ucout[3] = {c3, c2, c1};
    for (int i = 0; i < 3; ++i) {
        const std::string p = "decoder.up" + std::to_string(i + 1) + ".";
        add_section(h, p + "low_conv.weight", {ucout[i], ucin[i], 1, 3});
        add_section(h, p + "low_conv.bias", {ucout[i]});
        add_section(h, p + "high_conv.conv.weight", {3 * ucout[i], ucin[i], 1, 3});
        add_section(h, p + "high_conv.conv.bias", {3 * ucout[i]});
    }
    add_section(h, "decoder.mask_conv.0.weight", {2, c1, 2, 2});
    add_section(h, "decoder.mask_conv.0.bias", {2});
    add_section(h, "decoder.mask_conv.1.gamma", {1, 1, 1, F});
    add_section(h, "decoder.mask_conv.1.beta", {1, 1, 1, F});
    add_section(h, "decoder.mask_conv.2.weight", {2});
    add_section(h, "decoder.mask_conv.3.weight", {2, 2, 1, 1});
    add_section(h, "decoder.mask_conv.3.bias", {2});
    add_section(h, "decoder.lsigmoid.slope", {F, 1, 1});
}

int LisennetFamily::create(const fe_config* cfg, fe_handle** out) {
    if (cfg->win_size > cfg->n_fft) return fail(FE_ERR_INVALID_ARG, "n_fft(%d) must be bigger than win_size(%d)", cfg->n_fft, cfg->win_size);
    const fe::LImpl* li = (cfg->channels == 16 && cfg->rf_blocks == 2 && cfg->n_fft == 512 && cfg->hop_size == 256) ? fe_limpl_h256() : nullptr;
    if (!li)
        return fail(FE_ERR_UNSUPPORTED_CONFIG, "no LiSenNet kernel compiled for num_channels=%d n_blocks=%d n_fft=%d hop=%d "
                    "(configs/others/lisennet.yaml is the compiled architecture)", cfg->channels, cfg->rf_blocks, cfg->n_fft, cfg->hop_size);
    fe_handle* h = new_handle(cfg, Dims{16, 0, 16, 32, 2, cfg->n_fft, cfg->hop_size, cfg->n_fft / 2, 0, 0, {0}});
    h->limpl = li;
    build_sections_lisennet(h);
    *out = h;
    return FE_OK;
}

// r6: the stream-batched middle's operands (lisennet_sb_kernels.hip.h, fe::LSbPk behind fe::LPk::TOTAL).  A fragments of the TRANSPOSED products in
// k4 order (fe_fragments.h), written by fn(tile, row, quad m, j, lane group lgk) for k-step 4 m + j: what that k index means (source / tap /
// channel group of a convolution, channel 4 lg + j, hidden unit ...) is each layer's own choice below and the kernel's B operand follows it.
void pack_weights_lisennet_sb(const Blob& S, fe::frag::Buffer& buf) {
    using Q = fe::LSbPk;
    const int SB = fe::LPk::TOTAL;
    auto packA = [&](int dst, int NT, int NQ, auto&& fn) {
        buf.tiles<fe::frag::kK4>(SB + dst, NT, 4 * NQ, [&](int t, int row, int k) { return fn(t, row, k / 16, (k / 4) % 4, k % 4); });
    };
    auto packR = [&](int dst, int NT, auto&& fn) { buf.rows(SB + dst, NT, fn); };          // per-row values [tile][16]
    const double kL2E = 1.4426950408889634;
    const float sR = (float)-kL2E, sN = (float)(2.0 * kL2E);       // sigma(v) = rcp(1 + exp2(sR v)), tanh(v) = 1 - 2 rcp(1 + exp2(sN v))
    // convolutions: k-step j of quad m, lane group lgk <-> pair 4 m + lgk = ((source s, tap df), channel group g), channel 4 g + j
    // DSConv (cout, cin, 2, KF): source = frame dt (0: the cached frame, 1: this frame)
    auto dsconv = [&](const std::string& key, int cin, int cout, int KF, int NQ, int dst_w, int dst_b) {
        const float* w = S(key + ".weight");
        const float* b = S(key + ".bias");
        const int G = cin / 4, NPAIR = 2 * KF * G;
        packA(dst_w, 1, NQ, [&](int, int row, int m, int j, int lgk) {
            const int pi = 4 * m + lgk;
            if (pi >= NPAIR || row >= cout) return 0.0f;
            const int s_ = pi / (KF * G), rem = pi % (KF * G), df = rem / G, g = rem % G, c = 4 * g + j;
            return w[((row * cin + c) * 2 + s_) * KF + df];
        });
        packR(dst_b, 1, [&](int, int row) { return row < cout ? b[row] : 0.0f; });
    };
    auto ds_norm = [&](const std::string& p, int cout, int FO, int dst_g, int dst_be, int dst_p) {
        const float* g = S(p + ".norm.gamma");
        const float* be = S(p + ".norm.beta");
        const float* pr = S(p + ".act.weight");
        for (int i = 0; i < FO; ++i) { buf[SB + dst_g + i] = g[i]; buf[SB + dst_be + i] = be[i]; }
        for (int i = 0; i < 16; ++i) buf[SB + dst_p + i] = i < cout ? pr[i] : 0.0f;
    };
    {   // conv_1 (4, 3, 1, 1): [c][o] | bias; per-frequency affine; PReLU
        const float* w = S("encoder.conv_1.0.weight");
        const float* b = S("encoder.conv_1.0.bias");
        for (int o = 0; o < 4; ++o) { for (int c = 0; c < 3; ++c) buf[SB + Q::C1_W + c * 4 + o] = w[o * 3 + c]; buf[SB + Q::C1_W + 12 + o] = b[o]; }
        const float* g = S("encoder.conv_1.1.gamma");
        const float* be = S("encoder.conv_1.1.beta");
        const float* pr = S("encoder.conv_1.2.weight");
        for (int i = 0; i < 257; ++i) { buf[SB + Q::C1_G + i] = g[i]; buf[SB + Q::C1_BE + i] = be[i]; }
        for (int i = 0; i < 4; ++i) buf[SB + Q::C1_P + i] = pr[i];
    }
    dsconv("encoder.conv_2.low_conv", 4, 8, 3, 2, Q::C2_LO, Q::C2_BL);
    dsconv("encoder.conv_2.high_conv", 4, 8, 5, 3, Q::C2_HI, Q::C2_BH);
    ds_norm("encoder.conv_2", 8, 128, Q::C2_G, Q::C2_BE, Q::C2_P);
    dsconv("encoder.conv_3.low_conv", 8, 12, 3, 3, Q::C3_LO, Q::C3_BL);
    dsconv("encoder.conv_3.high_conv", 8, 12, 5, 5, Q::C3_HI, Q::C3_BH);
    ds_norm("encoder.conv_3", 12, 64, Q::C3_G, Q::C3_BE, Q::C3_P);
    dsconv("encoder.conv_4.low_conv", 12, 16, 3, 5, Q::C4_LO, Q::C4_BL);
    dsconv("encoder.conv_4.high_conv", 12, 16, 5, 8, Q::C4_HI, Q::C4_BH);
    ds_norm("encoder.conv_4", 16, 32, Q::C4_G, Q::C4_BE, Q::C4_P);
    // USConv (O, 2 CX, 1, 3) over cat(x, skip): source 0 = x, 1 = skip; oc(tile, row) = the conv channel a row computes (-1: idle row)
    auto usconv = [&](const std::string& key, int CX, int NT, int NQ, int dst_w, int dst_b, auto&& oc) {
        const float* w = S(key + ".weight");
        const float* b = S(key + ".bias");
        const int G = CX / 4, NPAIR = 2 * 3 * G, cin = 2 * CX;
        packA(dst_w, NT, NQ, [&](int t, int row, int m, int j, int lgk) {
            const int pi = 4 * m + lgk, o = oc(t, row);
            if (pi >= NPAIR || o < 0) return 0.0f;
            const int s_ = pi / (3 * G), rem = pi % (3 * G), df = rem / G, g = rem % G, c = 4 * g + j;
            return w[(o * cin + s_ * CX + c) * 3 + df];
        });
        packR(dst_b, NT, [&](int t, int row) { const int o = oc(t, row); return o >= 0 ? b[o] : 0.0f; });
    };
    // the pixel shuffle (SPConvTranspose2d, :240-246): out[c][3 w + phase] = conv[phase * cout + c][w]
    usconv("decoder.up1.low_conv", 16, 1, 6, Q::U1_LO, Q::U1_BL, [](int, int row) { return row < 12 ? row : -1; });
    usconv("decoder.up1.high_conv.conv", 16, 3, 6, Q::U1_HI, Q::U1_BH, [](int t, int row) { return row < 12 ? 12 * t + row : -1; });      // tile = phase
    usconv("decoder.up2.low_conv", 12, 1, 5, Q::U2_LO, Q::U2_BL, [](int, int row) { return row < 8 ? row : -1; });
    usconv("decoder.up2.high_conv.conv", 12, 2, 5, Q::U2_HI, Q::U2_BH, [](int t, int row) { return 16 * t + row < 24 ? 16 * t + row : -1; });   // rows 8 phase + c
    usconv("decoder.up3.low_conv", 8, 1, 3, Q::U3_LO, Q::U3_BL, [](int, int row) { return row < 4 ? row : -1; });
    usconv("decoder.up3.high_conv.conv", 8, 1, 3, Q::U3_HI, Q::U3_BH, [](int, int row) { return row < 12 ? row : -1; });                      // rows 4 phase + c
    {   // mask_conv.0 (2, 4, 2, 2): source = frame (0: cached, 1: this), two taps, one channel group; the rest of the mask head per bin / per channel
        dsconv("decoder.mask_conv.0", 4, 2, 2, 1, Q::M0_W, Q::M0_B);
        const float* g = S("decoder.mask_conv.1.gamma");
        const float* be = S("decoder.mask_conv.1.beta");
        const float* sl = S("decoder.lsigmoid.slope");
        for (int i = 0; i < 257; ++i) { buf[SB + Q::M_G + i] = g[i]; buf[SB + Q::M_BE + i] = be[i]; buf[SB + Q::M_SL + i] = sl[i]; }
        const float* pr = S("decoder.mask_conv.2.weight");
        buf[SB + Q::M_P] = pr[0]; buf[SB + Q::M_P + 1] = pr[1];
        const float* w3 = S("decoder.mask_conv.3.weight");         // (2, 2, 1, 1): [o][c]
        const float* b3 = S("decoder.mask_conv.3.bias");
        for (int i = 0; i < 4; ++i) buf[SB + Q::M3 + i] = w3[i];
        buf[SB + Q::M3 + 4] = b3[0]; buf[SB + Q::M3 + 5] = b3[1];
    }
    for (int blk = 0; blk < 2; ++blk) {
        const int D = Q::BLK + blk * Q::B_SIZE;
        const std::string p = "blocks." + std::to_string(blk) + ".";
        auto copy = [&](const std::string& n, int dst, int cnt) { const float* w = S(n); for (int i = 0; i < cnt; ++i) buf[SB + dst + i] = w[i]; };
        copy(p + "dp_rnn_attn.intra_norm.weight", D + Q::N1W, 512);
        copy(p + "dp_rnn_attn.intra_norm.bias", D + Q::N1B, 512);
        for (int d = 0; d < 2; ++d) {
            const std::string sfx = d ? "_reverse" : "";
            const std::string q_ = p + "dp_rnn_attn.intra_rnn_attn.rnn.";
            const float* wi = S(q_ + "weight_ih_l0" + sfx);        // (36, 16), gates r, z, n
            const float* wh = S(q_ + "weight_hh_l0" + sfx);        // (36, 12)
            const float* bi = S(q_ + "bias_ih_l0" + sfx);
            const float* bh = S(q_ + "bias_hh_l0" + sfx);
            for (int q = 0; q < 4; ++q) {
                const int wv = 4 * d + q;
                // the wave's tile: row 4 u' + g = (unit 3 q + u', gate g of r, z, n_x, n_h); quad 0: x (channel 4 lgk + j), quad 1: h (unit 4 j + lgk)
                packA(D + Q::I_W + wv * 2 * 256, 1, 2, [&](int, int row, int m, int j, int lgk) {
                    const int up = row / 4, g = row % 4, unit = 3 * q + up;
                    if (up >= 3) return 0.0f;
                    if (m == 0) {
                        const int c = 4 * lgk + j;
                        return g == 0 ? sR * wi[unit * 16 + c] : g == 1 ? sR * wi[(12 + unit) * 16 + c] : g == 2 ? sN * wi[(24 + unit) * 16 + c] : 0.0f;
                    }
                    const int hu = 4 * j + lgk;
                    if (j >= 3) return 0.0f;
                    return g == 0 ? sR * wh[unit * 12 + hu] : g == 1 ? sR * wh[(12 + unit) * 12 + hu] : g == 3 ? sN * wh[(24 + unit) * 12 + hu] : 0.0f;
                });
                packR(D + Q::I_B + wv * 16, 1, [&](int, int row) {
                    const int up = row / 4, g = row % 4, unit = 3 * q + up;
                    if (up >= 3) return 0.0f;
                    return g == 0 ? sR * (bi[unit] + bh[unit]) : g == 1 ? sR * (bi[12 + unit] + bh[12 + unit]) : g == 2 ? sN * bi[24 + unit] : sN * bh[24 + unit];
                });
            }
        }
        {
            const float* w = S(p + "dp_rnn_attn.intra_rnn_attn.dense.weight");     // (16, 24): input = [forward h | backward h]
            const float* b = S(p + "dp_rnn_attn.intra_rnn_attn.dense.bias");
            packA(D + Q::D1_W, 1, 2, [&](int, int row, int m, int j, int lgk) { return j < 3 ? w[row * 24 + m * 12 + 4 * j + lgk] : 0.0f; });
            packR(D + Q::D1_B, 1, [&](int, int row) { return b[row]; });
        }
        copy(p + "dp_rnn_attn.inter_norm.weight", D + Q::N2W, 512);
        copy(p + "dp_rnn_attn.inter_norm.bias", D + Q::N2B, 512);
        {
            const std::string q_ = p + "dp_rnn_attn.inter_rnn_attn.rnn.";
            const float* wi = S(q_ + "weight_ih_l0");              // (72, 16)
            const float* wh = S(q_ + "weight_hh_l0");              // (72, 24)
            const float* bi = S(q_ + "bias_ih_l0");
            const float* bh = S(q_ + "bias_hh_l0");
            // tile t: row <-> unit 16 t + row (< 24); quad 0: x (channel 4 lgk + j), quads 1, 2: h (unit 16 (quad - 1) + 4 lgk + j)
            auto gate_xh = [&](int dst, int g0, float sc) {
                packA(dst, 2, 3, [&](int t, int row, int m, int j, int lgk) {
                    const int u = 16 * t + row;
                    if (u >= 24) return 0.0f;
                    if (m == 0) return sc * wi[(g0 + u) * 16 + 4 * lgk + j];
                    const int hu = 16 * (m - 1) + 4 * lgk + j;
                    return hu < 24 ? sc * wh[(g0 + u) * 24 + hu] : 0.0f;
                });
            };
            gate_xh(D + Q::XR, 0, sR);
            gate_xh(D + Q::XZ, 24, sR);
            packA(D + Q::XNX, 2, 1, [&](int t, int row, int, int j, int lgk) { const int u = 16 * t + row; return u < 24 ? sN * wi[(48 + u) * 16 + 4 * lgk + j] : 0.0f; });
            packA(D + Q::XNH, 2, 2, [&](int t, int row, int m, int j, int lgk) {
                const int u = 16 * t + row, hu = 16 * m + 4 * lgk + j;
                return (u < 24 && hu < 24) ? sN * wh[(48 + u) * 24 + hu] : 0.0f;
            });
            packR(D + Q::XB, 8, [&](int gt, int row) {
                const int g = gt / 2, u = 16 * (gt % 2) + row;
                if (u >= 24) return 0.0f;
                return g == 0 ? sR * (bi[u] + bh[u]) : g == 1 ? sR * (bi[24 + u] + bh[24 + u]) : g == 2 ? sN * bi[48 + u] : sN * bh[48 + u];
            });
            const float* w = S(p + "dp_rnn_attn.inter_rnn_attn.dense.weight");     // (16, 24)
            const float* b = S(p + "dp_rnn_attn.inter_rnn_attn.dense.bias");
            packA(D + Q::D2_W, 1, 2, [&](int, int row, int m, int j, int lgk) { const int hu = 16 * m + 4 * lgk + j; return hu < 24 ? w[row * 24 + hu] : 0.0f; });
            packR(D + Q::D2_B, 1, [&](int, int row) { return b[row]; });
        }
        {
            const float* g = S(p + "conv_glu.norm.gamma");         // (1, 16, 1, 32): [d][f] -> [f][d]
            const float* be = S(p + "conv_glu.norm.beta");
            for (int f = 0; f < 32; ++f)
                for (int d = 0; d < 16; ++d) { buf[SB + D + Q::GG + f * 16 + d] = g[d * 32 + f]; buf[SB + D + Q::GBE + f * 16 + d] = be[d * 32 + f]; }
            const float* w1 = S(p + "conv_glu.fc1.weight");        // (64, 16, 1, 1)
            const float* b1 = S(p + "conv_glu.fc1.bias");
            packA(D + Q::F1_W, 4, 1, [&](int t, int row, int, int j, int lgk) { return w1[(16 * t + row) * 16 + 4 * lgk + j]; });
            packR(D + Q::F1_B, 4, [&](int t, int row) { return b1[16 * t + row]; });
            const float* dw = S(p + "conv_glu.dwconv.weight");     // (32, 1, 3, 3): [ch][dt][df] -> [t][r][q][lg][e], tap dt * 3 + df = 4 q + e of channel 16 t + 4 lg + r
            const float* db = S(p + "conv_glu.dwconv.bias");
            for (int t = 0; t < 2; ++t)
                for (int r = 0; r < 4; ++r)
                    for (int k = 0; k < 9; ++k)
                        for (int lg = 0; lg < 4; ++lg) buf[SB + D + Q::DW + ((t * 4 + r) * 3 + k / 4) * 16 + lg * 4 + k % 4] = dw[(16 * t + 4 * lg + r) * 9 + k];
            for (int e = 0; e < 32; ++e) buf[SB + D + Q::DWB + e] = db[e];
            const float* w2 = S(p + "conv_glu.fc2.weight");        // (16, 32, 1, 1)
            const float* b2 = S(p + "conv_glu.fc2.bias");
            packA(D + Q::F2_W, 1, 2, [&](int, int row, int m, int j, int lgk) { return w2[row * 32 + 16 * m + 4 * lgk + j]; });
            packR(D + Q::F2_B, 1, [&](int, int row) { return b2[row]; });
        }
    }
}

// k-major repack at the compile-time offsets of fe::LPk (lisennet_kernels.hip.h)
int LisennetFamily::pack_weights(fe_handle* h, const Blob& S, std::vector<float>* out) {
    using P = fe::LPk;
    fe::frag::Buffer buf(P::TOTAL + fe::LSbPk::TOTAL);
    auto copy = [&](const std::string& n, int dst, int cnt) { buf.raw(dst, cnt, S(n)); };
    pack_stft_tables(buf, h, P::WINDOW, P::WINDOW_I, P::TW);
    {
        const float* w = S("encoder.conv_1.0.weight");            // (4, 3, 1, 1) -> [c][o]
        for (int o = 0; o < 4; ++o) for (int c = 0; c < 3; ++c) buf[P::C1_W + c * 4 + o] = w[o * 3 + c];
        copy("encoder.conv_1.0.bias", P::C1_B, 4);
        copy("encoder.conv_1.1.gamma", P::C1_G, 257);
        copy("encoder.conv_1.1.beta", P::C1_BE, 257);
        copy("encoder.conv_1.2.weight", P::C1_P, 4);
    }
    // Conv2d (O, Cin, KT, KF) -> [((c*KT + dt)*KF + df)][O]
    auto conv = [&](const std::string& key, int O, int Cin, int KT, int KF, int dst_w, int dst_b) {
        const float* w = S(key + ".weight");
        for (int o = 0; o < O; ++o)
            for (int c = 0; c < Cin; ++c)
                for (int dt = 0; dt < KT; ++dt)
                    for (int df = 0; df < KF; ++df) buf[dst_w + ((c * KT + dt) * KF + df) * O + o] = w[((o * Cin + c) * KT + dt) * KF + df];
        if (dst_b >= 0) copy(key + ".bias", dst_b, O);
    };
    auto dsconv = [&](const std::string& p, int cin, int cout, int half, int lo, int hi, int bl, int bh, int g, int be, int pr) {
        conv(p + ".low_conv", cout, cin, 2, 3, lo, bl);
        conv(p + ".high_conv", cout, cin, 2, 5, hi, bh);
        copy(p + ".norm.gamma", g, 2 * half);
        copy(p + ".norm.beta", be, 2 * half);
        copy(p + ".act.weight", pr, cout);
    };
    dsconv("encoder.conv_2", 4, 8, 64, P::D2_LO, P::D2_HI, P::D2_BL, P::D2_BH, P::D2_G, P::D2_BE, P::D2_P);
    dsconv("encoder.conv_3", 8, 12, 32, P::D3_LO, P::D3_HI, P::D3_BL, P::D3_BH, P::D3_G, P::D3_BE, P::D3_P);
    dsconv("encoder.conv_4", 12, 16, 16, P::D4_LO, P::D4_HI, P::D4_BL, P::D4_BH, P::D4_G, P::D4_BE, P::D4_P);
    for (int b = 0; b < 2; ++b) {
        const int D = P::BLK + b * P::B_SIZE;
        const std::string p = "blocks." + std::to_string(b) + ".";
        copy(p + "dp_rnn_attn.intra_norm.weight", D + P::B_N1W, 512);
        copy(p + "dp_rnn_attn.intra_norm.bias", D + P::B_N1B, 512);
        for (int d = 0; d < 2; ++d) {
            const std::string sfx = d ? "_reverse" : "";
            const std::string q = p + "dp_rnn_attn.intra_rnn_attn.rnn.";
            const float* wi = S(q + "weight_ih_l0" + sfx);        // (36, 16)
            const float* wh = S(q + "weight_hh_l0" + sfx);        // (36, 12)
            const float* bi = S(q + "bias_ih_l0" + sfx);
            const float* bh = S(q + "bias_hh_l0" + sfx);
            for (int g = 0; g < 36; ++g) {
                for (int k = 0; k < 16; ++k) buf[D + P::B_IH + (d * 16 + k) * 36 + g] = wi[g * 16 + k];
                buf[D + P::B_GB + d * 36 + g] = bi[g] + (g < 24 ? bh[g] : 0.0f);
            }
            for (int gate = 0; gate < 3; ++gate)
                for (int k = 0; k < 12; ++k)
                    for (int c = 0; c < 12; ++c) buf[D + P::B_HH + ((d * 3 + gate) * 12 + k) * 12 + c] = wh[(gate * 12 + c) * 12 + k];
            for (int c = 0; c < 12; ++c) buf[D + P::B_HN + d * 12 + c] = bh[24 + c];
        }
        {
            const float* w = S(p + "dp_rnn_attn.intra_rnn_attn.dense.weight");     // (16, 24) -> [k][d]
            for (int d = 0; d < 16; ++d) for (int k = 0; k < 24; ++k) buf[D + P::B_D1W + k * 16 + d] = w[d * 24 + k];
            copy(p + "dp_rnn_attn.intra_rnn_attn.dense.bias", D + P::B_D1B, 16);
        }
        copy(p + "dp_rnn_attn.inter_norm.weight", D + P::B_N2W, 512);
        copy(p + "dp_rnn_attn.inter_norm.bias", D + P::B_N2B, 512);
        {
            const std::string q = p + "dp_rnn_attn.inter_rnn_attn.rnn.";
            const float* wi = S(q + "weight_ih_l0");              // (72, 16)
            const float* wh = S(q + "weight_hh_l0");              // (72, 24)
            const float* bi = S(q + "bias_ih_l0");
            const float* bh = S(q + "bias_hh_l0");
            for (int g = 0; g < 72; ++g) {
                for (int k = 0; k < 16; ++k) buf[D + P::B_XIH + k * 72 + g] = wi[g * 16 + k];
                for (int k = 0; k < 24; ++k) buf[D + P::B_XHH + k * 72 + g] = wh[g * 24 + k];
                buf[D + P::B_XGB + g] = bi[g] + (g < 48 ? bh[g] : 0.0f);
            }
            for (int c = 0; c < 24; ++c) buf[D + P::B_XHN + c] = bh[48 + c];
            const float* w = S(p + "dp_rnn_attn.inter_rnn_attn.dense.weight");
            for (int d = 0; d < 16; ++d) for (int k = 0; k < 24; ++k) buf[D + P::B_D2W + k * 16 + d] = w[d * 24 + k];
            copy(p + "dp_rnn_attn.inter_rnn_attn.dense.bias", D + P::B_D2B, 16);
        }
        copy(p + "conv_glu.norm.gamma", D + P::B_GG, 512);        // (1, 16, 1, 32) -> [d][f]
        copy(p + "conv_glu.norm.beta", D + P::B_GBE, 512);
        {
            const float* w = S(p + "conv_glu.fc1.weight");        // (64, 16, 1, 1) -> [d][o]
            for (int o = 0; o < 64; ++o) for (int d = 0; d < 16; ++d) buf[D + P::B_F1W + d * 64 + o] = w[o * 16 + d];
            copy(p + "conv_glu.fc1.bias", D + P::B_F1B, 64);
            const float* dw = S(p + "conv_glu.dwconv.weight");    // (32, 1, 3, 3) -> [(dt*3 + df)][ch]
            for (int c = 0; c < 32; ++c) for (int j = 0; j < 9; ++j) buf[D + P::B_DW + j * 32 + c] = dw[c * 9 + j];
            copy(p + "conv_glu.dwconv.bias", D + P::B_DWB, 32);
            const float* w2 = S(p + "conv_glu.fc2.weight");       // (16, 32, 1, 1) -> [ch][d]
            for (int d = 0; d < 16; ++d) for (int c = 0; c < 32; ++c) buf[D + P::B_F2W + c * 16 + d] = w2[d * 32 + c];
            copy(p + "conv_glu.fc2.bias", D + P::B_F2B, 16);
        }
    }
    conv("decoder.up1.low_conv", 12, 32, 1, 3, P::U1_LO, P::U1_BL);
    conv("decoder.up1.high_conv.conv", 36, 32, 1, 3, P::U1_HI, P::U1_BH);
    conv("decoder.up2.low_conv", 8, 24, 1, 3, P::U2_LO, P::U2_BL);
    conv("decoder.up2.high_conv.conv", 24, 24, 1, 3, P::U2_HI, P::U2_BH);
    conv("decoder.up3.low_conv", 4, 16, 1, 3, P::U3_LO, P::U3_BL);
    conv("decoder.up3.high_conv.conv", 12, 16, 1, 3, P::U3_HI, P::U3_BH);
    conv("decoder.mask_conv.0", 2, 4, 2, 2, P::M0_W, P::M0_B);
    copy("decoder.mask_conv.1.gamma", P::M_G, 257);
    copy("decoder.mask_conv.1.beta", P::M_BE, 257);
    copy("decoder.mask_conv.2.weight", P::M_P, 2);
    {
        const float* w = S("decoder.mask_conv.3.weight");          // (2, 2, 1, 1) -> [c][o]
        for (int o = 0; o < 2; ++o) for (int c = 0; c < 2; ++c) buf[P::M3_W + c * 2 + o] = w[o * 2 + c];
        copy("decoder.mask_conv.3.bias", P::M3_B, 2);
        copy("decoder.lsigmoid.slope", P::SLOPE, 257);
    }
    pack_weights_lisennet_sb(S, buf);
    *out = std::move(buf.v);
    return FE_OK;
}

fe::LStreamArgs LisennetFamily::args(fe_handle* h, int B, int T) {
    fe::LStreamArgs a{};
    a.wp = h->packed_dev;
    a.B = B;
    a.T = T;
    a.compression = h->cfg.input_compression;
    return a;
}

// LiSenNet per-hop step of large batches: conv_3 .. up3 batched over the streams (lisennet_sb_kernels.hip.h) from "lisennet_stream_batch_min" streams
// (0 = never).  The carry (fe::LCarry: the tiles' activation tensors + the compressed spectra) is grow-only scratch of the handle.
int LisennetFamily::ensure_sb(fe_handle* h, int B) {
    return ensure_sb_scratch(h, B, h->opt[OPT_LISENNET_SB_MIN], fe::LCarry::floats(B) * sizeof(float));
}

// Every launch of the per-stream kernel.  The plain flavour may grow the stream-batched scratch and run the per-hop step of a large batch through
// it; the slotted and packet flavours (fe_step_pool, fe_step_pool_streams[_pinned]) run the per-stream kernel in their own instantiation at every
// batch size (the stream-batched middle's tensors are laid out per call tile) and allocate nothing.
int LisennetFamily::launch_step(fe_handle* h, fe::LStreamArgs& a, fe::StepFlavour flavour, void* stream) {
    hipError_t e = hipSuccess;
    const int sb_min = h->opt[OPT_LISENNET_SB_MIN];
    if (flavour == fe::STEP_PLAIN && a.mode == fe::FE_MODE_STREAM && a.T == 1 && sb_min > 0 && a.B >= sb_min && h->limpl->launch_sb) {
        const int rc = ensure_sb(h, a.B);
        if (rc != FE_OK) return rc;
        a.carry = h->sb_dev;
        h->limpl->launch_sb(a, h->max_wgs, (hipStream_t)stream, &e);
        return launch_rc(e);
    }
    h->limpl->launch_step(a, flavour, h->max_wgs, (hipStream_t)stream, &e);
    return launch_rc(e);
}

const char* LisennetFamily::stage_name(const fe_handle*, int idx) {
    static const char* const names[16] = {"spec_in", "compressed", "features", "encoder.conv_1", "encoder.conv_2", "encoder.conv_3", "encoder.conv_4",
                                          "blocks.0.intra", "blocks.0.inter", "blocks.0", "blocks.1.intra", "blocks.1.inter", "blocks.1",
                                          "decoder.up3", "mask", "spec_out"};
    return names[idx];
}

double LisennetFamily::macs(const fe_handle*) {   // models/lisennet/macs.py:8-66 with T = 1
    const double C = 16, Nb = 2, F1 = 257;
    double m = 3 * (C / 4) * F1;
    const double co[3] = {C / 2, C / 4 * 3, C}, fi[3] = {257, 128, 64};
    for (int i = 0; i < 3; ++i) {
        const double f = fi[i], fq = std::floor(f / 4), fhi = std::floor((f - fq + 2 - 5) / 3) + 1;
        m += (2 * 3 * fq + 2 * 5 * fhi) * co[i] * co[i];
    }
    auto gru = [](double i, double hd) { return (i + hd) * hd * 3 + hd * 3; };
    const double hh = 24, ff = 32;
    for (int b = 0; b < (int)Nb; ++b) {
        m += (gru(C, hh / 2) * 2 + hh * C + gru(C, hh) + hh * C) * ff;
        m += (C * C * 4 + C * 2 * 3 + C * 2 + C * 2 * C) * ff;
    }
    double c_in = C, f = 32, c_out = 0;
    for (double c_o : {C / 4 * 3, C / 2, C / 4}) { c_out = c_o; m += (3 * (f / 2) + 3 * 3 * (f / 2)) * c_in * 2 * c_out; c_in = c_out; f *= 2; }
    f += 1;
    m += (c_out * 2 * 2 * 2 + 2 * 2 + 2 * 2) * f;
    return m;
}
