// The body of conv5_kernel (csrc/conv5x5.hip) and conv5_dgrad_kernel (csrc/conv5x5_grad.hip): included between the braces of
// a __global__ function with the parameter `Conv5Params p` and `using Side = Conv5Fwd` or `Conv5Dgrad`
// (conv5x5_common.hpp says why it is included and not called).  Side::mirror (a compile-time constant: every `if
// constexpr` and `?:` on it below is resolved before code generation, nothing is tested at run time) marks the four places
// where the data gradient differs: the patch origin and a patch pixel's predicate, the prepared kernel row of a stage, the
// prepared column of a tap, the epilogue.
    extern __shared__ float4 c5_lds[];
    u32x4* As = reinterpret_cast<u32x4*>(c5_lds);
    u32x4* Ws = As + 2 * C5_ABUF;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = wave_id();
    const int l31 = lane & 31, lhi = lane >> 5;
    const int mh = wave & 1, nh = wave >> 1;
    const int pcol = c5_pcol(l31);
    const float ca = pow2_scale_of(*p.amag);
    const float oscale = (1.f / ca) * (1.f / *p.wscale);
    const int nchunks = p.K16;

    const C5Tile tl = c5_tile<C5_TS, C5_TS>(blockIdx.x, p.nct, p.tiles_x, p.tiles_y);
    const int ct = tl.ct, x0 = tl.x0, y0 = tl.y0, n = tl.n;

    // ---- staging of a patch chunk: unit u = (pixel u / 2, octet u % 2), 32 contiguous bytes ----
    const long long aelems = (long long)p.N * p.Ha * p.Wa * p.lda;
    const int rbase = Side::mirror && y0 > 4 ? y0 - 4 : 0;
    long long afirst;
    if constexpr (Side::mirror) afirst = (((long long)n * p.Ha + rbase) * p.Wa) * p.lda;
    else afirst = (((long long)n * p.Ha + y0) * p.Wa + x0) * p.lda;
    const rsrc_t ra = c5_rsrc(p.a + afirst, (aelems - afirst) * 4);
    const rsrc_t rnone = c5_rsrc(p.a, 0);
    u32x4 areg[C5_AROUNDS][2];
    unsigned avoff[C5_AROUNDS];
#pragma unroll
    for (int j = 0; j < C5_AROUNDS; ++j) {
        const int u = tid + 256 * j, q = u >> 1, half = u & 1;
        const int qr = q / C5_PS, qc = q - qr * C5_PS;
        if constexpr (Side::mirror) {
            const int gy = y0 - 4 + qr, gc = x0 - 4 + qc;
            const bool in = u < 2 * C5_PP && gy >= 0 && gy < p.Ha && gc >= 0 && gc < p.Wa;
            avoff[j] = in ? (unsigned)(((gy - rbase) * p.Wa + gc) * p.lda + half * 8) * 4u : C5_OOB;
        } else {
            const bool in = u < 2 * C5_PP && y0 + qr < p.Ha && x0 + qc < p.Wa;
            avoff[j] = in ? (unsigned)((qr * p.Wa + qc) * p.lda + half * 8) * 4u : C5_OOB;
        }
    }
    // (valid = false: a request beyond the last chunk -- an empty descriptor, every lane reads zero.  No load of the main
    // loop sits under a branch: at a control-flow join the compiler waits for ALL outstanding loads.)
    auto issue_a = [&](int cc, bool valid) {
        const rsrc_t r = valid ? ra : rnone;
#pragma unroll
        for (int j = 0; j < C5_AROUNDS; ++j)
#pragma unroll
            for (int i = 0; i < 2; ++i)
                areg[j][i] = __builtin_amdgcn_raw_buffer_load_b128(r, avoff[j], (unsigned)cc * 64u + 16u * i, 0);
    };
    auto commit_a = [&](int abuf) {
#pragma unroll
        for (int j = 0; j < C5_AROUNDS; ++j) {
            const int u = tid + 256 * j, q = u >> 1, half = u & 1;
            if (u < 2 * C5_PP) {
                u32x4 hh, ll;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const unsigned w0 = areg[j][c / 2][(2 * c) % 4];
                    const unsigned w1 = areg[j][c / 2][(2 * c + 1) % 4];
                    unsigned hp, lp;
                    f16_split_pair(__builtin_bit_cast(float, w0), __builtin_bit_cast(float, w1), ca, hp, lp);
                    hh[c] = hp;
                    ll[c] = lp;
                }
                u32x4* d = As + abuf * C5_ABUF + half * C5_PR + q;
                d[0] = hh;
                d[2 * C5_PR] = ll;
            }
        }
    };
    // ---- staging of a weight stage (chunk cc, PREPARED kernel row kr): 2560 entries, 10 per thread ----
    const long long wentries = (long long)p.nct * p.K16 * 5 * C5_WSTAGE;
    const rsrc_t rw = c5_rsrc(p.wp, wentries * 16);
    u32x4 wreg[C5_WROUNDS];
    auto issue_w = [&](int cc, int kr, bool valid) {
        const rsrc_t r = valid ? rw : rnone;
        const unsigned block = valid ? (unsigned)((ct * p.K16 + cc) * 5 + kr) : 0u;
#pragma unroll
        for (int i = 0; i < C5_WROUNDS; ++i)
            wreg[i] = __builtin_amdgcn_raw_buffer_load_b128(r, (unsigned)(tid + 256 * i) * 16u,
                                                            block * (unsigned)(C5_WSTAGE * 16), 0);
    };
    auto commit_w = [&](int wbuf) {
#pragma unroll
        for (int i = 0; i < C5_WROUNDS; ++i) Ws[wbuf * C5_WSTAGE + tid + 256 * i] = wreg[i];
    };

    // Two accumulator sets: hx hw in one, the cross products hx lw + lx hw -- 2^-11 of it and smaller -- in the other,
    // added once in the epilogue.  Every MFMA rounds its accumulator: with all three products in one set the sum of
    // 25 K16 terms is rounded 75 K16 times at its full magnitude, this way 25 K16 times (the cross sums' roundings are
    // 2^-11 of that).  One wave per SIMD owns 512 registers: 256 accumulators fit.
    f32x16 acc[4][2], acx[4][2];
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mi][ni][r] = acx[mi][ni][r] = 0.f;

    // operands of one tap: A 4 m-blocks x 2 planes, B 2 n-blocks x 2 planes
    struct Ops { u32x4 ah[4], al[4], bh[2], bl[2]; };
    // tap i of a stage: the patch shifted by i entries against prepared column Side::kcol(i)
    auto load_ops = [&](Ops& o, const u32x4* Ab, const u32x4* Wb, int i) {
        const int kc = Side::mirror ? 4 - i : i;
        o.bh[0] = Wb[kc * 512];
        o.ah[0] = Ab[i];
        o.bh[1] = Wb[kc * 512 + 32];
#pragma unroll
        for (int mi = 1; mi < 4; ++mi) o.ah[mi] = Ab[mi * 2 * C5_PS + i];
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) o.bl[ni] = Wb[kc * 512 + 256 + ni * 32];
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) o.al[mi] = Ab[2 * C5_PR + mi * 2 * C5_PS + i];
    };
    auto mfmas = [&](const Ops& o) {
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = c5_mfma(o.ah[mi], o.bh[ni], acc[mi][ni]);
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) acx[mi][ni] = c5_mfma(o.ah[mi], o.bl[ni], acx[mi][ni]);
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) acx[mi][ni] = c5_mfma(o.al[mi], o.bh[ni], acx[mi][ni]);
    };
    // the next tap's 12 operand fetches go BETWEEN the current tap's 24 MFMAs (2 MFMAs, 1 fetch, ...)
    auto interleave = [&]() {
#pragma unroll
        for (int i = 0; i < 12; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);      // MFMA
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);      // DS read
        }
    };
    // this lane's operand addresses in patch buffer 0 / weight buffer 0 (octet = k half = lane / 32)
    const u32x4* const a_lane = As + lhi * C5_PR + (mh * 8 + (l31 >> 4)) * C5_PS + pcol;
    const u32x4* const w_lane = Ws + lhi * C5_NT + nh * 64 + l31;

    // ---- prologue: chunk 0's patch and its first stage ----
    issue_a(0, true);
    issue_w(0, Side::mirror ? 4 : 0, true);
    commit_a(0);
    commit_w(0);
    __syncthreads();

    // Stage s = 5 cc + j reads patch buffer cc % 2 at row offset j, prepared kernel row Side::krow(j) and weight buffer
    // s % 2.  The weights of stage s + 1 are requested at its start and written to buffer (s + 1) % 2 -- last read in stage
    // s - 1, before the previous barrier -- at its end; the patch of chunk cc + 1 is requested at the start of stage j = 3
    // and written at the end of stage j = 4.  Every j (and tap i) is a constant where it is used: the Side's rows and
    // columns cost nothing in the loop.
    for (int cc = 0; cc < nchunks; ++cc) {
        const bool more = cc + 1 < nchunks;
        const u32x4* const Ac = a_lane + (cc & 1) * C5_ABUF;
        auto stage = [&](const int j) {
            const int s = cc * 5 + j;
            if (j < 4) issue_w(cc, Side::mirror ? 3 - j : j + 1, true);
            else issue_w(cc + 1, Side::mirror ? 4 : 0, more);
            if (j == 3) issue_a(cc + 1, more);
            const u32x4* Ab = Ac + j * C5_PS;
            const u32x4* Wb = w_lane + (s & 1) * C5_WSTAGE;
            Ops o0, o1;
            load_ops(o0, Ab, Wb, 0);
            load_ops(o1, Ab, Wb, 1);
            mfmas(o0);
            interleave();
            load_ops(o0, Ab, Wb, 2);
            mfmas(o1);
            interleave();
            load_ops(o1, Ab, Wb, 3);
            mfmas(o0);
            interleave();
            load_ops(o0, Ab, Wb, 4);
            mfmas(o1);
            interleave();
            mfmas(o0);
            if (j == 4) commit_a((cc + 1) & 1);
            commit_w((s + 1) & 1);
            __syncthreads();
        };
        stage(0);
        stage(1);
        stage(2);
        stage(3);
        stage(4);
    }

    // ---- epilogue: the Side's value of every sum, largest magnitude, masked stores ----
    const long long yelems = (long long)p.N * p.Hy * p.Wy * p.ldy;
    const long long yfirst = (((long long)n * p.Hy + y0) * p.Wy + x0) * p.ldy;
    const rsrc_t ry = c5_rsrc(p.y + yfirst, (yelems - yfirst) * 4);
    const bool undo = Side::mirror && p.aux != nullptr;
    const rsrc_t rs = undo ? c5_rsrc(p.aux + yfirst, (yelems - yfirst) * 4) : rnone;
    float bv[2];
    int ch[2];
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
        ch[ni] = ct * C5_NT + nh * 64 + ni * 32 + l31;
        if constexpr (!Side::mirror) bv[ni] = ch[ni] < p.Cout ? p.aux[ch[ni]] : 0.f;
    }
    unsigned amax_run = 0;
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = mh * 8 + mi * 2 + c5_acc_row(r);
            const int col = c5_acc_col(r, lhi);
            const bool ok = y0 + row < p.Hy && x0 + col < p.Wy;
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) {
                const bool st = ok && ch[ni] < p.ldy;
                const unsigned voff = st ? (unsigned)((row * p.Wy + col) * p.ldy + ch[ni]) * 4u : C5_OOB;
                float v;
                if constexpr (Side::mirror) {
                    const float saved = buf_load(rs, voff, 0);
                    v = (acc[mi][ni][r] + acx[mi][ni][r]) * oscale;
                    v = (undo && !(saved > 0.f)) ? v * p.slope : v;
                } else {
                    v = (acc[mi][ni][r] + acx[mi][ni][r]) * oscale + bv[ni];
                    v = v > 0.f ? v : v * p.slope;
                }
                if (st) {
                    const unsigned a = abits(v);
                    amax_run = amax_run > a ? amax_run : a;
                }
                buf_store(v, ry, voff, 0);
            }
        }
    }
    if (p.amax) amax_publish(amax_run, p.amax);          // (wave-uniform condition; a barrier inside)
