// fe_api_bsrnn.inc - host side of the BSRNN family: weight sections, handle creation, packer, launch (included by fe_api.hip inside its anonymous namespace)
// ============================================================================ BSRNN (models/bsrnn/model.py)
const int kSub[31] = {2, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 16, 16, 16, 16, 16, 16, 16, 17};

// The family as fe_api.hip's shared baseline-family paths see it (visit_baseline: the stream and spec steps, offline, the buffer sizes, debug stages)
struct BsrnnFamily {
    using Args = fe::BArgs;
    using StreamArgs = fe::BStreamArgs;
    static const fe::BImpl* impl(const fe_handle* h) { return h->bimpl; }
    static const char* shape_name(const fe_handle* h) { return h->bimpl->name; }
    static float*& state(Args& a) { return a.lstm; }
    static size_t state_floats(const fe_handle* h, int B) { return (size_t)2 * h->cfg.rf_blocks * B * 31 * 2 * h->cfg.channels; }
    // the model's state of `cap` streams as regions from float `off` on (state_regions): h0, c0, h1, c1, ... [2 L][cap][31 * 2C]
    static int regions(const fe_handle* h, size_t, size_t off, StateRegion* r) {
        r[0] = {off, 2 * h->cfg.rf_blocks, 31 * 2 * h->cfg.channels};
        return 1;
    }
    static size_t counters(const fe_handle* h) { return h->cfg.rf_blocks; }      // time-pipeline frame counters per stream
    // default frames in flight per utterance of a time-pipelined offline launch: a hand-off chain (wait, fetch, gate GEMM, publish) is ~1/40
    // of a frame, so every co-resident workgroup the batch leaves free is worth having
    static constexpr int kPipeFrames = 64;
    static constexpr bool kPipeCarriesState = true;      // (fe_step_backlog: the PIPE kernel's frames hand the streaming state on in place)
    static constexpr bool kPipeCarriesStateOnRequest = false;      // (it always does: nothing to ask for)
    static size_t ring_floats(const fe_handle*) { return 0; }
    static void set_ring(Args&, float*) {}
    static size_t xp_floats(const fe_handle* h) { return (size_t)h->max_wgs * h->bimpl->xp_floats; }     // (band-LSTM input projections of C = 64)
    static StreamArgs args(fe_handle* h, int B, int T);
    static int create(const fe_config* cfg, fe_handle** out);
    static int pack_weights(fe_handle* h, const Blob& S, std::vector<float>* out);
    static int ensure_sb(fe_handle* h, int B);
    static int launch_step(fe_handle* h, StreamArgs& a, fe::StepFlavour flavour, void* stream);
    static const char* stage_name(const fe_handle* h, int idx);
    static double macs(const fe_handle* h);
};

void build_sections_bsrnn(fe_handle* h) {
    const int C = h->cfg.channels, L = h->cfg.rf_blocks, HH = 2 * C;
    char nm[160];
    for (int b = 0; b < 31; ++b) {
        snprintf(nm, sizeof nm, "band_split.fc.%d.weight", b); add_section(h, nm, {C, 2 * kSub[b], 1});
        snprintf(nm, sizeof nm, "band_split.fc.%d.bias", b); add_section(h, nm, {C});
    }
    for (int l = 0; l < L; ++l) {
        snprintf(nm, sizeof nm, "rnn_time.%d.weight_ih", l); add_section(h, nm, {4 * HH, C});
        snprintf(nm, sizeof nm, "rnn_time.%d.weight_hh", l); add_section(h, nm, {4 * HH, HH});
        snprintf(nm, sizeof nm, "rnn_time.%d.bias_ih", l); add_section(h, nm, {4 * HH});
        snprintf(nm, sizeof nm, "rnn_time.%d.bias_hh", l); add_section(h, nm, {4 * HH});
        snprintf(nm, sizeof nm, "fc_time.%d.weight", l); add_section(h, nm, {C, HH});
        snprintf(nm, sizeof nm, "fc_time.%d.bias", l); add_section(h, nm, {C});
        for (const char* sfx : {"", "_reverse"}) {
            snprintf(nm, sizeof nm, "rnn_freq.%d.weight_ih_l0%s", l, sfx); add_section(h, nm, {4 * HH, C});
            snprintf(nm, sizeof nm, "rnn_freq.%d.weight_hh_l0%s", l, sfx); add_section(h, nm, {4 * HH, HH});
            snprintf(nm, sizeof nm, "rnn_freq.%d.bias_ih_l0%s", l, sfx); add_section(h, nm, {4 * HH});
            snprintf(nm, sizeof nm, "rnn_freq.%d.bias_hh_l0%s", l, sfx); add_section(h, nm, {4 * HH});
        }
        snprintf(nm, sizeof nm, "fc_freq.%d.weight", l); add_section(h, nm, {C, 2 * HH});
        snprintf(nm, sizeof nm, "fc_freq.%d.bias", l); add_section(h, nm, {C});
    }
    for (const char* kind : {"mlp_mask", "mlp_residual"})
        for (int b = 0; b < 31; ++b) {
            snprintf(nm, sizeof nm, "mask_decoder.%s.%d.0.weight", kind, b); add_section(h, nm, {4 * C, C, 1});
            snprintf(nm, sizeof nm, "mask_decoder.%s.%d.0.bias", kind, b); add_section(h, nm, {4 * C});
            snprintf(nm, sizeof nm, "mask_decoder.%s.%d.2.weight", kind, b); add_section(h, nm, {4 * kSub[b], 4 * C, 1});
            snprintf(nm, sizeof nm, "mask_decoder.%s.%d.2.bias", kind, b); add_section(h, nm, {4 * kSub[b]});
        }
}

int BsrnnFamily::create(const fe_config* cfg, fe_handle** out) {
    if (cfg->n_fft != 512) return fail(FE_ERR_INVALID_ARG, "Only n_fft=512 is supported, but given %d", cfg->n_fft);
    if (cfg->win_size > cfg->n_fft) return fail(FE_ERR_INVALID_ARG, "n_fft(%d) must be bigger than win_size(%d)", cfg->n_fft, cfg->win_size);
    if (cfg->hop_size <= 0 || cfg->hop_size > cfg->n_fft) return fail(FE_ERR_INVALID_ARG, "hop_size %d out of range", cfg->hop_size);
    const fe::BImpl* bi = nullptr;
    for (const fe::BImpl* im : bimpls())
        if (im->C == cfg->channels && im->NLAY == cfg->rf_blocks && im->HOP == cfg->hop_size) bi = im;
    if (!bi)
        return fail(FE_ERR_UNSUPPORTED_CONFIG, "no BSRNN kernel compiled for num_channels=%d num_layers=%d hop=%d", cfg->channels,
                    cfg->rf_blocks, cfg->hop_size);
    fe_handle* h = new_handle(cfg, Dims{cfg->channels, 0, 0, 0, cfg->rf_blocks, cfg->n_fft, cfg->hop_size, cfg->n_fft / 2, 0, 0, {0}});
    h->bimpl = bi;
    build_sections_bsrnn(h);
    *out = h;
    return FE_OK;
}

// Grows in allocation order: the offsets it hands out are BOffsets / SbOffsets.  Fragment orders: fe_fragments.h
int BsrnnFamily::pack_weights(fe_handle* h, const Blob& S, std::vector<float>* out) {
    const int C = h->cfg.channels, L = h->cfg.rf_blocks, HH = 2 * C, G4 = 4 * HH, R = 4 * 257;
    const bool whh_regs = h->bimpl->whh_regs;
    fe::BOffsets& o = h->boff;
    fe::frag::Buffer buf;
    auto pack_b = [&](int K, int Ncols, auto&& Bkn) {
        const int off = buf.alloc((size_t)((Ncols + 15) / 16) * (K / 4) * 64);
        buf.pack_b(off, K, Ncols, Bkn);
        return off;
    };
    // LSTM gate rows (order i, f, g, o) are packed pre-scaled: with pre' = s_g * pre the kernel evaluates every gate as
    // rcp(1 + exp2(pre')): sigma(v) for s = -log2(e), and tanh(v) = 2 rcp(1 + exp2(-2 log2(e) v)) - 1 for the cell gate g
    const double kL2E = 1.4426950408889634;
    auto gscale = [&](int row) { return (float)((row / HH) == 2 ? -2.0 * kL2E : -kL2E); };
    char nm[160];
    {   // band split: [k/4][band*C + c] float4 - thread (band, c) reads its zero-padded row as 16-byte loads coalesced over the threads
        o.bs_w = buf.alloc((size_t)31 * C * fe::kBsKP);
        o.bs_b = buf.alloc(31 * C);
        for (int b = 0; b < 31; ++b) {
            snprintf(nm, sizeof nm, "band_split.fc.%d.weight", b);
            const float* w = S(nm);                                   // (C, 2sub)
            const int k2 = 2 * kSub[b];
            for (int c = 0; c < C; ++c)
                for (int k = 0; k < k2; ++k) buf[o.bs_w + (((size_t)(k / 4) * 31 * C) + b * C + c) * 4 + (k & 3)] = w[c * k2 + k];
            snprintf(nm, sizeof nm, "band_split.fc.%d.bias", b);
            buf.raw(o.bs_b + b * C, C, S(nm));
        }
    }
    for (int l = 0; l < L; ++l) {
        auto key = [&](const char* fmt) { snprintf(nm, sizeof nm, fmt, l); return std::string(nm); };
        {   // time LSTM: K = [x (C) | h (HH)], N = 4HH gate rows (i,f,g,o)
            const float* wih = S(key("rnn_time.%d.weight_ih"));
            const float* whh = S(key("rnn_time.%d.weight_hh"));
            o.t_w[l] = pack_b(C + HH, G4, [&](int k, int n) { return gscale(n) * (k < C ? wih[n * C + k] : whh[n * HH + (k - C)]); });
            const float* bi = S(key("rnn_time.%d.bias_ih"));
            const float* bh = S(key("rnn_time.%d.bias_hh"));
            o.t_b[l] = buf.alloc(G4);
            for (int i = 0; i < G4; ++i) buf[o.t_b[l] + i] = gscale(i) * (bi[i] + bh[i]);
        }
        {
            const float* w = S(key("fc_time.%d.weight"));         // (C, HH)
            o.tfc_w[l] = pack_b(HH, C, [&](int k, int n) { return w[n * HH + k]; });
            o.tfc_b[l] = buf.alloc(C);
            buf.raw(o.tfc_b[l], C, S(key("fc_time.%d.bias")));
        }
        for (int d = 0; d < 2; ++d) {
            const char* sfx = d ? "_reverse" : "";
            auto keyd = [&](const char* stem) { snprintf(nm, sizeof nm, "rnn_freq.%d.%s_l0%s", l, stem, sfx); return std::string(nm); };
            const float* wih = S(keyd("weight_ih"));
            o.f_wih[l][d] = pack_b(C, G4, [&](int k, int n) { return gscale(n) * wih[n * C + k]; });
            const float* bi = S(keyd("bias_ih"));
            const float* bh = S(keyd("bias_hh"));
            o.f_b[l][d] = buf.alloc(G4);
            for (int i = 0; i < G4; ++i) buf[o.f_b[l][d] + i] = gscale(i) * (bi[i] + bh[i]);
            {   // recurrence weights in thread order.  Thread t (0..NTD-1; NTD = 128, or 256 for C = 64) of a direction = 4 u + q, hidden unit u (+ NTD/4 rr).
                // KSPLIT shapes: q = K-quarter; the thread holds, for all four gates g, W_hh[g*HH + u + 32 rr][q*HH/4 + kk] at
                //   [rr][g*HH/4 + kk][t].  Otherwise q = gate: it holds row W_hh[q*HH + u + 32 rr][k] at [rr][k][t].
                // (streamed shapes: the k index in float4 groups)
                const float* whh = S(keyd("weight_hh"));      // (4HH, HH), gate-major rows
                o.f_whh[l][d] = buf.alloc((size_t)G4 * HH);
                const int NTD = h->bimpl->rec_threads, UPP = NTD / 4;      // threads of a direction (256 for C = 64: SEQD), units per pass
                const int RPT = HH / UPP, Q = HH / 4;
                const bool ksplit = h->bimpl->ksplit;
                for (int rr = 0; rr < RPT; ++rr)
                    for (int kp = 0; kp < HH; ++kp)
                        for (int t = 0; t < NTD; ++t) {
                            const int u = (t >> 2) + UPP * rr, q = t & 3;
                            const int row = ksplit ? (kp / Q) * HH + u : q * HH + u;
                            const int k = ksplit ? q * Q + (kp % Q) : kp;
                            const float v = gscale(row) * whh[(size_t)row * HH + k];
                            if (whh_regs) buf[o.f_whh[l][d] + ((size_t)rr * HH + kp) * NTD + t] = v;
                            else buf[o.f_whh[l][d] + ((((size_t)rr * (HH / 4)) + kp / 4) * NTD + t) * 4 + (kp & 3)] = v;
                        }
            }
        }
        {
            const float* w = S(key("fc_freq.%d.weight"));         // (C, 2HH)
            o.ffc_w[l] = pack_b(2 * HH, C, [&](int k, int n) { return w[n * 2 * HH + k]; });
            o.ffc_b[l] = buf.alloc(C);
            buf.raw(o.ffc_b[l], C, S(key("fc_freq.%d.bias")));
        }
    }
    if (h->bimpl->launch_sb) {
        // stream-batched layers (bsrnn_sb_kernels.hip.h): the weights as A fragments of the TRANSPOSED products.  Feature permutations:
        // k-step ks, lane group lg carries channel KSC lg + ks / hidden unit KSH lg + ks; row 4 lg' + r of gate tile t = (unit KSH lg' + t,
        // gate r); row 4 lg' + r of fc output tile `to` = channel KSC lg' + 4 to + r.
        fe::SbOffsets& so = h->sboff;
        const int KSC = C / 4, KSH = HH / 4, KS1 = KSC + KSH, NTO = C / 16;
        auto pack_lstm = [&](const float* wih, const float* whh, const float* bi, const float* bh, int* w_off, int* b_off) {
            *w_off = buf.alloc((size_t)KSH * KS1 * 64);
            *b_off = buf.alloc((size_t)KSH * 16);
            auto row = [&](int t, int rho) { return (rho % 4) * HH + KSH * (rho / 4) + t; };
            buf.tiles(*w_off, KSH, KS1, [&](int t, int rho, int k) {
                const int ks = k / 4, lgk = k % 4, rw = row(t, rho);
                return gscale(rw) * (ks < KSC ? wih[(size_t)rw * C + KSC * lgk + ks] : whh[(size_t)rw * HH + KSH * lgk + (ks - KSC)]);
            });
            buf.rows(*b_off, KSH, [&](int t, int rho) { return gscale(row(t, rho)) * (bi[row(t, rho)] + bh[row(t, rho)]); });
        };
        auto chan = [&](int to, int rho) { return KSC * (rho / 4) + 4 * to + rho % 4; };
        auto pack_fc = [&](const float* w, int ld, int col0, int* w_off) {       // rows = channels, columns col0 .. col0 + HH - 1 of a (C, ld) matrix
            *w_off = buf.alloc((size_t)NTO * KSH * 64);
            buf.tiles(*w_off, NTO, KSH, [&](int to, int rho, int k) { return w[(size_t)chan(to, rho) * ld + col0 + KSH * (k % 4) + k / 4]; });
        };
        // k-steps [k0, k0 + nk) of a packed matrix's tiles once more, in k4 order
        auto k4_copy = [&](int src, int ntiles, int kst, int k0, int nk) {
            const int dst = buf.alloc((size_t)ntiles * nk * 64);
            buf.regroup_k4(dst, src, ntiles, kst, k0, nk);
            return dst;
        };
        auto pack_fc_bias = [&](const float* b, int* b_off) {
            *b_off = buf.alloc((size_t)NTO * 16);
            buf.rows(*b_off, NTO, [&](int to, int rho) { return b[chan(to, rho)]; });
        };
        for (int l = 0; l < L; ++l) {
            auto key = [&](const char* fmt) { snprintf(nm, sizeof nm, fmt, l); return std::string(nm); };
            pack_lstm(S(key("rnn_time.%d.weight_ih")), S(key("rnn_time.%d.weight_hh")), S(key("rnn_time.%d.bias_ih")), S(key("rnn_time.%d.bias_hh")), &so.t_w[l], &so.t_b[l]);
            so.t_w4[l] = C == 64 ? k4_copy(so.t_w[l], KSH, KS1, 0, KS1) : 0;
            pack_fc(S(key("fc_time.%d.weight")), HH, 0, &so.tfc_w[l]);
            so.tfc_w4[l] = C == 64 ? k4_copy(so.tfc_w[l], NTO, KSH, 0, KSH) : 0;
            pack_fc_bias(S(key("fc_time.%d.bias")), &so.tfc_b[l]);
            for (int d = 0; d < 2; ++d) {
                const char* sfx = d ? "_reverse" : "";
                auto keyd = [&](const char* stem) { snprintf(nm, sizeof nm, "rnn_freq.%d.%s_l0%s", l, stem, sfx); return std::string(nm); };
                pack_lstm(S(keyd("weight_ih")), S(keyd("weight_hh")), S(keyd("bias_ih")), S(keyd("bias_hh")), &so.f_w[l][d], &so.f_b[l][d]);
                if (C == 64) {      // bsrnn_sb64_layers_kernel: x k-steps (streamed every step) and h k-steps in k4 order
                    so.f_wx4[l][d] = k4_copy(so.f_w[l][d], KSH, KS1, 0, KSC);
                    so.f_wh4[l][d] = k4_copy(so.f_w[l][d], KSH, KS1, KSC, KSH);
                } else so.f_wx4[l][d] = so.f_wh4[l][d] = 0;
                pack_fc(S(key("fc_freq.%d.weight")), 2 * HH, d * HH, &so.ffc_w[l][d]);
                so.ffc_w4[l][d] = C == 64 ? k4_copy(so.ffc_w[l][d], NTO, KSH, 0, KSH) : 0;
            }
            pack_fc_bias(S(key("fc_freq.%d.bias")), &so.ffc_b[l]);
        }
    }
    const char* kinds[2] = {"mlp_mask", "mlp_residual"};
    for (int kind = 0; kind < 2; ++kind) {
        o.m_w1[kind] = buf.alloc((size_t)31 * 4 * C * C);      // [band][k/4][o] float4
        o.m_b1[kind] = buf.alloc((size_t)31 * 4 * C);
        o.m_w2[kind] = buf.alloc((size_t)R * 4 * C);           // [k/4][global row] float4
        o.m_b2[kind] = buf.alloc(R);
        int row0 = 0;
        for (int b = 0; b < 31; ++b) {
            snprintf(nm, sizeof nm, "mask_decoder.%s.%d.0.weight", kinds[kind], b);
            {
                const float* w1 = S(nm);                                  // (4C, C) -> [k/4][o] float4 per band
                for (int oo = 0; oo < 4 * C; ++oo)
                    for (int k = 0; k < C; ++k)
                        buf[o.m_w1[kind] + (((size_t)b * (C / 4) + k / 4) * (4 * C) + oo) * 4 + (k & 3)] = w1[oo * C + k];
            }
            snprintf(nm, sizeof nm, "mask_decoder.%s.%d.0.bias", kinds[kind], b);
            buf.raw(o.m_b1[kind] + b * 4 * C, 4 * C, S(nm));
            snprintf(nm, sizeof nm, "mask_decoder.%s.%d.2.weight", kinds[kind], b);
            const int rows = 4 * kSub[b];
            {
                const float* w2 = S(nm);                                  // (4sub, 4C) -> [k/4][global row] float4
                for (int r = 0; r < rows; ++r)
                    for (int k = 0; k < 4 * C; ++k)
                        buf[o.m_w2[kind] + ((size_t)(k / 4) * R + row0 + r) * 4 + (k & 3)] = w2[r * 4 * C + k];
            }
            snprintf(nm, sizeof nm, "mask_decoder.%s.%d.2.bias", kinds[kind], b);
            buf.raw(o.m_b2[kind] + row0, rows, S(nm));
            row0 += rows;
        }
    }
    {   // index tables (ints stored in the float buffer): band of a layer-2 row; a bin's first value row and 2*sub of its band
        o.row_band = buf.alloc(R);
        o.bin_row = buf.alloc(257);
        o.bin_2sub = buf.alloc(257);
        int row0 = 0, f0 = 0;
        for (int b = 0; b < 31; ++b) {
            for (int r = 0; r < 4 * kSub[b]; ++r) { const int v = b; memcpy(&buf[o.row_band + row0 + r], &v, 4); }
            for (int f = 0; f < kSub[b]; ++f) {
                const int ra = 4 * f0 + 2 * f, s2 = 2 * kSub[b];
                memcpy(&buf[o.bin_row + f0 + f], &ra, 4);
                memcpy(&buf[o.bin_2sub + f0 + f], &s2, 4);
            }
            row0 += 4 * kSub[b];
            f0 += kSub[b];
        }
    }
    o.window = buf.alloc(h->window.size()); o.window_istft = buf.alloc(h->window_istft.size()); o.twiddle = buf.alloc(h->twiddle.size());
    pack_stft_tables(buf, h, o.window, o.window_istft, o.twiddle);
    if (C == 16) {
        // r5: the role-split PART 1's copies, regrouped from the sections packed above for 16-byte fetches (see BOffsets)
        const int KSC = C / 4, KSH = HH / 4, KS1 = KSC + KSH, NCT = HH / 16;
        for (int l = 0; l < L; ++l) {
            o.ov_t[l] = buf.alloc((size_t)NCT * 4 * KS1 * 64);       // tile ct * 4 + g <- the time LSTM's column tile g * NCT + ct
            buf.regroup_k4(o.ov_t[l], o.t_w[l], NCT * 4, KS1, 0, KS1, [&](int t) { return (t % 4) * NCT + t / 4; });
            o.ov_tx[l] = buf.alloc((size_t)NCT * 4 * 16 * C);
            for (int ct = 0; ct < NCT; ++ct)
                for (int g = 0; g < 4; ++g)
                    for (int r = 0; r < 16; ++r)
                        for (int ch = 0; ch < C; ++ch)
                            buf[o.ov_tx[l] + (((size_t)(ct * 4 + g) * 16 + r) * C) + ch] = buf[o.t_w[l] + ((size_t)(g * NCT + ct) * KS1 + ch / 4) * 64 + (ch % 4) * 16 + r];
            o.ov_f1t[l] = buf.alloc((size_t)C * HH);
            for (int ch = 0; ch < C; ++ch)
                for (int un = 0; un < HH; ++un) buf[o.ov_f1t[l] + (size_t)ch * HH + un] = buf[o.tfc_w[l] + (size_t)(un / 4) * 64 + (un % 4) * 16 + ch];
            o.ov_f2[l] = buf.alloc((size_t)2 * KSH * 64);
            buf.regroup_k4(o.ov_f2[l], o.ffc_w[l], 1, 2 * KSH, 0, 2 * KSH);
            for (int d = 0; d < 2; ++d) {
                // row-major for the transposed chains: W[n][ch] = fragment (tile n / 16, k-step ch / 4) lane (ch % 4) * 16 + n % 16
                o.ov_ipt[l][d] = buf.alloc((size_t)G4 * C);
                for (int n = 0; n < G4; ++n)
                    for (int ch = 0; ch < C; ++ch)
                        buf[o.ov_ipt[l][d] + (size_t)n * C + ch] = buf[o.f_wih[l][d] + ((size_t)(n / 16) * KSC + ch / 4) * 64 + (ch % 4) * 16 + n % 16];
                // W_hh: lane = half * 32 + unit holds gate rows (half, 2 + half) of its unit; source [k][4 u + gate] (register shapes, NTD = 128)
                o.ov_hh[l][d] = buf.alloc((size_t)2 * (HH / 4) * 256);
                for (int rs = 0; rs < 2; ++rs)
                    for (int q = 0; q < HH / 4; ++q)
                        for (int lane = 0; lane < 64; ++lane)
                            for (int j = 0; j < 4; ++j) {
                                const int half = lane >> 5, u = lane & 31, gate = 2 * rs + half, k = 4 * q + j;
                                buf[o.ov_hh[l][d] + (((size_t)rs * (HH / 4) + q) * 64 + lane) * 4 + j] = buf[o.f_whh[l][d] + (size_t)k * 128 + 4 * u + gate];
                            }
            }
        }
    }
    {   // the matrix-core DFT's constant operands (r5: the role-split PART 1 runs the STFT on them), N = 512: N1 = 16, KC = 8, MT = 1
        const int N1 = h->cfg.n_fft / 32, KC = N1 / 2, MT = N1 / 16;
        o.dft1 = buf.alloc(2 * 2 * 8 * 64); o.dft2 = buf.alloc((size_t)2 * KC * 64); o.dft3 = buf.alloc((size_t)2 * MT * KC * 64); o.dft4 = buf.alloc(2 * 2 * 8 * 64);
        pack_dft_constants(buf, h->cfg.n_fft, o.dft1, o.dft2, o.dft3, o.dft4);
    }
    o.total = (int)((buf.size() + 63) & ~(size_t)63);
    h->packed_floats = o.total;
    buf.v.resize(o.total, 0.0f);
    *out = std::move(buf.v);
    return FE_OK;
}

fe::BStreamArgs BsrnnFamily::args(fe_handle* h, int B, int T) {
    fe::BStreamArgs a{};
    a.xp_scratch = h->skip_dev;
    a.wp = h->packed_dev;
    a.off = h->boff;
    a.B = B;
    a.T = T;
    a.compression = h->cfg.input_compression;
    return a;
}

// The per-hop BSRNN step runs as three launches (bsrnn_kernels.hip.h, PART): per stream 31 C floats of band features, 514 of compressed
// spectrum and 2056 of MLP pre-activations pass through the stream-batched scratch.  Grow-only; fe_state_init sizes it for its batch, so that a
// steady-state step allocates nothing (FE_BSRNN_SPLIT=0: the fused kernel, for A/B measurements).
constexpr int kSyncTiles = 64;       // sixteen-stream tiles of a fused BSRNN step (one workgroup per CU: 1024 CUs)
size_t bsplit_floats_per_stream(const fe_handle* h) {
    return (size_t)31 * h->cfg.channels + 2 * 257 + 2 * 1028 + (h->bimpl->launch_sb ? (size_t)2 * 31 * 2 * h->cfg.channels : 0);      // (+ the stream-batched layers' y scratch)
}
int BsrnnFamily::ensure_sb(fe_handle* h, int B) {
    // (bsrnn_three_launch_step is 0 or 1: the three-launch step, when it is on, takes the scratch from one stream on)
    const int rc = ensure_sb_scratch(h, B, h->opt[OPT_BSRNN_THREE_LAUNCH], (size_t)B * bsplit_floats_per_stream(h) * sizeof(float));
    if (rc != FE_OK || !h->sb_dev || h->bsync_dev) return rc;
    FE_HIP_CHECK(hipMalloc(&h->bsync_dev, kSyncTiles * 2 * sizeof(unsigned int)));
    FE_HIP_CHECK(hipMemset(h->bsync_dev, 0, kSyncTiles * 2 * sizeof(unsigned int)));
    return FE_OK;
}

// Every launch of the per-stream kernels, with the plan of the step made here.  The plain flavour (fe_step and the debug / profile steps,
// fe_spec_step, fe_offline) may grow the stream-batched scratch and take the three-launch step from it, the stream-batched layers, the fused step or
// the role-split profile.  The slotted and packet flavours (fe_step_pool, fe_step_pool_streams[_pinned]: always streaming steps) run the per-stream
// kernels that choice leaves, in their own instantiations: never the stream-batched layers or the fused step (their tensors are laid out per call
// tile), and nothing is allocated - the three-launch step runs where the scratch fe_state_init sized holds the call's streams, as it does for fe_step
// after that call; without it the single-kernel walk.
int BsrnnFamily::launch_step(fe_handle* h, fe::BStreamArgs& a, fe::StepFlavour flavour, void* stream) {
    hipError_t e = hipSuccess;
    const bool plain = flavour == fe::STEP_PLAIN;
    a.ov_off = (h->step_kernel == FE_STEP_KERNEL_WAVES4 || !h->opt[OPT_BSRNN_ROLE_SPLIT]) ? 1 : 0;
    bool split = a.mode == fe::FE_MODE_STREAM && a.T == 1;
    if (split && plain) {
        // (fe_set_option("bsrnn_ov_profile", 1): fe_profile_step probes the role-split PART 1 of the three-launch step instead of the fused kernel's phases)
        const bool ov_prof = h->opt[OPT_BSRNN_OV_PROFILE] != 0;
        split = a.dbg == nullptr && (a.clk == nullptr || (ov_prof && h->cfg.channels == 16 && a.B <= h->max_wgs));
        if (split) {
            const int rc = ensure_sb(h, a.B);
            if (rc != FE_OK) return rc;
        }
    }
    split = split && h->sb_dev && a.B <= h->sb_streams;
    if (split) {
        a.mlp_x = h->sb_dev;
        a.mlp_sp = a.mlp_x + (size_t)a.B * 31 * h->cfg.channels;
        a.mlp_pre = a.mlp_sp + (size_t)a.B * 2 * 257;
    }
    if (split && plain) {
        a.sb_y = a.mlp_pre + (size_t)a.B * 2 * 1028;
        a.gsync = (h->opt[OPT_BSRNN_FUSED] && a.clk == nullptr && (a.B + 15) / 16 <= kSyncTiles) ? h->bsync_dev : nullptr;
        // large batches: the LSTM layers batched over the streams on the matrix cores (sixteen streams per workgroup) - from the batch
        // size where sixteen-stream workgroups fill the chip better than one stream per workgroup (FE_BSRNN_SB: that threshold; 0 = never)
        // (default 2048; measured crossover on 256 CUs: ~1900 streams, profiles/r4c_bsrnn_stream_batched.txt.  num_channels = 64 (r6): a sixteen-stream tile takes 5.8 ms
        //  whatever the batch and the per-stream kernel 2.3 us per stream - crossover at ~2700 streams: the threshold counts 11 / 8 there)
        const int sb_opt = h->opt[OPT_BSRNN_SB_MIN];
        const int sb_min = h->cfg.channels == 64 ? (int)((long long)sb_opt * 11 / 8) : sb_opt;
        if (h->bimpl->launch_sb && sb_min > 0 && a.B >= sb_min) {
            h->bimpl->launch_sb(a, h->sboff, h->packed_floats, h->max_wgs, (hipStream_t)stream, &e);
            return launch_rc(e);
        }
    }
    h->bimpl->launch_step(a, flavour, split, h->max_wgs, (hipStream_t)stream, &e);
    return launch_rc(e);
}

// spec_in, compressed, band_split, (layer.l.time, layer.l.freq)..., mask_mlp, spec_out
const char* BsrnnFamily::stage_name(const fe_handle* h, int idx) {
    static thread_local std::string nm;
    const int L = h->cfg.rf_blocks;
    char bufn[64];
    if (idx == 0) nm = "spec_in";
    else if (idx == 1) nm = "compressed";
    else if (idx == 2) nm = "band_split";
    else if (idx < 3 + 2 * L) { snprintf(bufn, sizeof bufn, (idx - 3) % 2 == 0 ? "layer.%d.time" : "layer.%d.freq", (idx - 3) / 2); nm = bufn; }
    else if (idx == 3 + 2 * L) nm = "mask_mlp";
    else nm = "spec_out";
    return nm.c_str();
}

double BsrnnFamily::macs(const fe_handle* h) {   // models/bsrnn/macs.py:18-51
    const double C = h->cfg.channels, Hh = 2 * C, Lr = h->cfg.rf_blocks;
    double m = 0;
    for (int b = 0; b < 31; ++b) m += 2 * kSub[b] * C;
    m += (C * Hh * 4 + Hh * Hh * 4 + Hh * C + (C * Hh * 4 + Hh * Hh * 4) * 2 + 2 * Hh * C) * 31 * Lr;
    for (int b = 0; b < 31; ++b) m += (C * C * 4 + 4 * C * 4 * kSub[b]) * 2;
    return m;
}
