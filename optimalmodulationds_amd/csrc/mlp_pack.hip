// The host half of installing a distance network (omds_set_mlp_ex, network.hip): argument checks, zero-padding to the kernels'
// width and every MFMA fragment pack (MlpPacks, capi_internal.h).  No HIP runtime call in this file: the sanitizer build runs all
// of it on the CPU through the test hook at the end.
#include "capi_internal.h"
#ifdef OMDS_TEST_HOOKS
#include "omds_test.h"
#endif

// fp32 -> IEEE binary16 bits, round to nearest even (the screening network's weights, screen_kernel.hip)
uint16_t f32_to_f16_bits(float f) {
    uint32_t x;
    std::memcpy(&x, &f, 4);
    const uint32_t sign = (x >> 16) & 0x8000u;
    x &= 0x7fffffffu;
    if (x >= 0x7f800000u) return (uint16_t)(sign | 0x7c00u | ((x > 0x7f800000u) ? 0x200u : 0u));   // inf / nan
    if (x >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);                                        // rounds to >= 65520: inf
    if (x < 0x38800000u) {                                                                          // subnormal half or zero
        if (x < 0x33000000u) return (uint16_t)sign;                                                 // < 2^-25: zero
        const int shift = 126 - (int)(x >> 23);                                                     // 14 .. 24
        const uint32_t mant = (x & 0x7fffffu) | 0x800000u;
        const uint32_t q = mant >> shift, rem = mant & ((1u << shift) - 1u), halfway = 1u << (shift - 1);
        return (uint16_t)(sign | (q + ((rem > halfway || (rem == halfway && (q & 1u))) ? 1u : 0u)));
    }
    const uint32_t e = (x >> 23) - 112u, mant = x & 0x7fffffu;
    uint32_t h = (e << 10) | (mant >> 13);
    const uint32_t rem = mant & 0x1fffu;
    if (rem > 0x1000u || (rem == 0x1000u && (h & 1u))) ++h;                                         // may carry into the exponent: correct
    return (uint16_t)(sign | h);
}

// fp16 screening network (screen_kernel.hip): slices of 32 output rows x 256 k in A-fragment order of v_mfma_f32_32x32x16_f16, with
// the k order permuted to the C layout of the previous layer (chunk cc, lane-half h, slot j <-> position 16cc + 8(j>>2) + 4h + (j&3)).
// Behind a skip concatenation (level L = output of Linear L) the consuming layer's input columns are packed in a VIRTUAL
// order: its own c0 = out_dims[L] columns first, the 3d concatenated input columns LAST (virtual 256 - 3d .. 255 = k-chunks
// 14 and 15 whatever c0 is -- the K order of a dot product is free), zeros in between: omds_screen_sidx puts the inputs there.
// order (optional, [nhh + 1][256]): order[L][p] = the hidden unit of Linear L that sits at POSITION p of the screening network --
// row p of that layer's slices, k position p of the layer behind it.  Any permutation computes the same function; the kernel
// skips k-chunks whose 16 units are zero for all pairs of a wave, so the units that seldom or never fire are put together
// (screen_reorder).  nullptr: the identity.
void build_screen_pack(MlpPacks& pk, const int32_t* order) {
    const int nhh = pk.nhh, C = pk.C, Wd = OMDS_WIDTH, F = 3 * pk.d, n_linear = nhh + 2;
    const uint32_t skip_mask = pk.skip_mask;
    std::vector<const float*> Wv(n_linear), bv(n_linear);
    for (int i = 0; i < n_linear; ++i) { Wv[i] = pk.host_W[i].data(); bv[i] = pk.host_b[i].data(); }
    const float* const* W = Wv.data();
    const float* const* b = bv.data();
    auto unit = [&](int L, int p) -> int { return order ? order[(size_t)L * Wd + p] : p; };   // position p of Linear L's outputs
    auto real_col = [&](int consumer, int v) -> int {   // virtual input position v of Linear `consumer` -> column of Wpad, -1 = zero
        const int L = consumer - 1;
        if (L < 0 || !((skip_mask >> L) & 1u)) return unit(L, v);
        const int c0 = pk.out_dims[L];
        if (v < c0) return v;
        if (v >= Wd - F) return c0 + (v - (Wd - F));
        return -1;
    };
    // tanh: every layer in front of an activation is scaled by 2 log2(e) (screen_kernel.hip: act_pk); the last layer is not
    const float hs = pk.act == OMDS_ACT_TANH ? OMDS_SCREEN_TANH_SCALE : 1.f;
    std::vector<uint16_t>& wh = pk.wh;
    const int nsl = nhh * 8 + 2;
    wh.assign((size_t)nsl * 16 * 64 * 8, 0);
    pk.sbias.assign((size_t)(nhh + 2) * Wd, 0.f);
    // slice 0: layer 1, fragment 2 fb + cc = positions 32 fb .. +31 x inputs 16 cc .. +15 (slot j of lane-half h = input 16cc + 8h + j)
    for (int fb = 0; fb < 8; ++fb)
        for (int cc = 0; cc < 2; ++cc)
            for (int lane = 0; lane < 64; ++lane)
                for (int j = 0; j < 8; ++j) {
                    const int r = unit(0, 32 * fb + (lane & 31)), kk = 16 * cc + 8 * (lane >> 5) + j;
                    const float v = (kk < F) ? W[0][(size_t)r * F + kk] : 0.f;
                    wh[(((size_t)(2 * fb + cc)) * 64 + lane) * 8 + j] = f32_to_f16_bits(hs * v);
                }
    for (int sl = 1; sl < nsl; ++sl) {
        const bool lastl = sl == nsl - 1;
        const int lin = lastl ? n_linear - 1 : (sl - 1) / 8 + 1;   // the Linear layer this slice belongs to
        const float* Wsrc = W[lin];
        const int fb = lastl ? 0 : (sl - 1) % 8, rows = lastl ? C : Wd;
        for (int cc = 0; cc < 16; ++cc)
            for (int lane = 0; lane < 64; ++lane)
                for (int j = 0; j < 8; ++j) {
                    const int rp = 32 * fb + (lane & 31), r = (lastl || rp >= Wd) ? rp : unit(lin, rp);
                    const int kk = real_col(lin, 16 * cc + 8 * (j >> 2) + 4 * (lane >> 5) + (j & 3));
                    const float v = (rp < rows && kk >= 0) ? Wsrc[(size_t)r * Wd + kk] : 0.f;
                    wh[(((size_t)sl * 16 + cc) * 64 + lane) * 8 + j] = f32_to_f16_bits(lastl ? v : hs * v);
                }
    }
    for (int L = 0; L <= nhh; ++L)
        for (int p = 0; p < Wd; ++p) pk.sbias[(size_t)L * Wd + p] = hs * b[L][unit(L, p)];
    std::memcpy(&pk.sbias[(size_t)(nhh + 1) * Wd], b[n_linear - 1], C * sizeof(float));
}
#define PREQ(cond, code, msg) do { if (!(cond)) { err = (msg); return (code); } } while (0)
// What the fused install (build_mlp_packs) and the wide one (network.hip: set_mlp_wide) both require of their arguments; the
// conditions only one of them has stay beside it.
int check_mlp_args(int n, int n_linear, const int32_t* in_dims, const int32_t* out_dims, const float* const* W, const float* const* b,
                   int act, float out_div, std::string& err) {
    PREQ(in_dims && out_dims && W && b && n_linear >= 2, OMDS_ERR_INVALID_ARG, "omds_set_mlp: null argument or fewer than 2 Linear layers");
    PREQ(in_dims[0] == 3 * (n + 3) || in_dims[0] == 3 * (n + 2), OMDS_ERR_INVALID_ARG,
         "omds_set_mlp: dims[0] must be 3*(n_dof+3), or 3*(n_dof+2) for planar obstacle points (NeRF encoding [x, sin x, cos x])");
    PREQ(in_dims[0] <= 32, OMDS_ERR_UNSUPPORTED, "omds_set_mlp: 3*(n_dof+3) > 32 not supported");
    PREQ(n_linear - 1 <= OMDS_MAX_HIDDEN, OMDS_ERR_UNSUPPORTED, "omds_set_mlp: too many hidden layers");
    const int C = out_dims[n_linear - 1];
    PREQ(C >= 1 && C <= OMDS_CPAD, OMDS_ERR_UNSUPPORTED, "omds_set_mlp: 1 <= out_channels <= 16 required");
    PREQ(act == OMDS_ACT_RELU || act == OMDS_ACT_TANH, OMDS_ERR_UNSUPPORTED, "omds_set_mlp: act must be OMDS_ACT_RELU or OMDS_ACT_TANH");
    PREQ(out_div != 0.f, OMDS_ERR_INVALID_ARG, "omds_set_mlp: out_div must be non-zero");
    for (int i = 0; i < n_linear; ++i) PREQ(W[i] && b[i], OMDS_ERR_INVALID_ARG, "omds_set_mlp: null weight or bias array");
    return OMDS_OK;
}

int build_mlp_packs(int n, int n_linear, const int32_t* in_dims, const int32_t* out_dims, const float* const* W,
                    const float* const* b, int act, float out_div, int n_skips, const int32_t* skip_after, MlpPacks& pk,
                    std::string& err) {
    int rc;
    if ((rc = check_mlp_args(n, n_linear, in_dims, out_dims, W, b, act, out_div, err))) return rc;
    PREQ(n_skips == 0 || skip_after, OMDS_ERR_INVALID_ARG, "omds_set_mlp_ex: n_skips > 0 needs skip_after");
    const int d = in_dims[0] / 3, nhid = n_linear - 1;
    uint32_t skip_mask = 0;   // bit i: the encoded input is concatenated behind the activations of Linear i (network_macros_mod.py:142-146)
    for (int s = 0; s < n_skips; ++s) {
        PREQ(skip_after[s] >= 0 && skip_after[s] < nhid, OMDS_ERR_INVALID_ARG,
             "omds_set_mlp_ex: skip_after entries must name a hidden Linear layer (0 .. n_linear-2)");
        skip_mask |= 1u << skip_after[s];
    }
    for (int i = 0; i < nhid; ++i)
        PREQ(out_dims[i] >= 1 && out_dims[i] + (((skip_mask >> i) & 1u) ? 3 * d : 0) <= OMDS_WIDTH, OMDS_ERR_UNSUPPORTED,
             "omds_set_mlp: hidden widths (plus a concatenated input) above 256 are not supported by the MFMA kernels (narrower layers are zero-padded to width 256)");
    for (int i = 1; i < n_linear; ++i)
        PREQ(in_dims[i] == out_dims[i - 1] + (((skip_mask >> (i - 1)) & 1u) ? 3 * d : 0), OMDS_ERR_INVALID_ARG,
             "omds_set_mlp: the input width of a Linear layer must be the previous output width (+ 3*(n_dof+3) behind a skip concatenation)");
    const int C = out_dims[n_linear - 1];
    // Narrower hidden layers (the reference also ships 128-wide nets) are zero-padded to the kernels' width:
    // padded units have zero weights and biases on both sides, so relu/tanh(0) = 0 feeds nothing forward and
    // receives no gradient -- outputs and gradients are unchanged (the padded MFMA work is wasted, not wrong).
    // A concatenated input keeps its place: its columns follow the (narrower) layer's own outputs in the padded row.
    std::vector<std::vector<float>> Wpad(n_linear), bpad(n_linear);
    std::vector<const float*> Wp(n_linear), bp(n_linear);
    for (int i = 0; i < n_linear; ++i) {
        const int in = in_dims[i], out = out_dims[i];
        const int pin = i == 0 ? in : OMDS_WIDTH, pout = i == n_linear - 1 ? out : OMDS_WIDTH;
        Wpad[i].assign((size_t)pout * pin, 0.f);
        bpad[i].assign((size_t)pout, 0.f);
        for (int o = 0; o < out; ++o) {
            std::memcpy(&Wpad[i][(size_t)o * pin], &W[i][(size_t)o * in], (size_t)in * sizeof(float));
            bpad[i][o] = b[i][o];
        }
        Wp[i] = Wpad[i].data();
        bp[i] = bpad[i].data();
    }
    W = Wp.data();
    b = bp.data();
    pk.nhh = nhid - 1;
    pk.C = C;
    pk.d = d;
    pk.out_div = out_div;
    pk.act = act;
    pk.skip_mask = skip_mask;
    for (int i = 0; i < nhid; ++i) pk.skip_col[i] = (uint8_t)(((skip_mask >> i) & 1u) ? out_dims[i] : 0);
    const int nhh = pk.nhh;
    const int Wd = OMDS_WIDTH;
    // hidden->hidden: forward and transposed (backward) fragment packs
    std::vector<float4>&wf = pk.wf, &wb = pk.wb;
    wf.assign((size_t)std::max(nhh, 1) * OMDS_NCB * 32 * 64, make_float4(0, 0, 0, 0));
    wb.assign(wf.size(), make_float4(0, 0, 0, 0));
    pk.bh.assign((size_t)std::max(nhh, 1) * Wd, 0.f);
    for (int l = 0; l < nhh; ++l) {
        const float* Wl = W[l + 1];
        for (int cb = 0; cb < OMDS_NCB; ++cb)
            for (int c = 0; c < 32; ++c)
                for (int lane = 0; lane < 64; ++lane) {
                    // the lane's fragment covers POSITIONS 8c + 4(lane>>5) .. +3 of the k-permuted tile: columns omds_kat(position)
                    const int j = 32 * cb + (lane & 31), s0 = 8 * c + 4 * (lane >> 5);
                    const int k0 = omds_kat(s0), k1 = omds_kat(s0 + 1), k2 = omds_kat(s0 + 2), k3 = omds_kat(s0 + 3);
                    const size_t o = (((size_t)l * OMDS_NCB + cb) * 32 + c) * 64 + lane;
                    wf[o] = make_float4(Wl[j * Wd + k0], Wl[j * Wd + k1], Wl[j * Wd + k2], Wl[j * Wd + k3]);
                    wb[o] = make_float4(Wl[k0 * Wd + j], Wl[k1 * Wd + j], Wl[k2 * Wd + j], Wl[k3 * Wd + j]);
                }
        std::memcpy(&pk.bh[(size_t)l * Wd], b[l + 1], Wd * sizeof(float));
    }
    // 16-row packs (v_mfma_f32_16x16x4): the four tile positions of lane group g in steps 0..3 of chunk c are
    // 16c + pa[g] + {0, 2, 8, 10}, pa = {0, 4, 1, 5} -- the position SEQUENCE of the 32-row kernels (8c'+{0,4,1,5,2,6,3,7}), i.e.
    // columns 16c + 0 .. 15 in ascending order (omds_kat), so a 16-row tile is bit-identical to a 32-row tile (both MFMAs are
    // fmaf chains in k order, tools/ubench/mfma_order.hip)
    auto k16 = [](int c, int g, int mm) { return omds_kat(16 * c + ((g >> 1) + 4 * (g & 1)) + 8 * (mm >> 1) + 2 * (mm & 1)); };
    std::vector<float4>&wf16 = pk.wf16, &wb16 = pk.wb16;
    wf16.assign(wf.size(), make_float4(0, 0, 0, 0));
    wb16.assign(wf.size(), make_float4(0, 0, 0, 0));
    for (int l = 0; l < nhh; ++l) {
        const float* Wl = W[l + 1];
        for (int cb = 0; cb < 16; ++cb)
            for (int c = 0; c < 16; ++c)
                for (int lane = 0; lane < 64; ++lane) {
                    const int j = 16 * cb + (lane & 15), g = lane >> 4;
                    const int k0 = k16(c, g, 0), k1 = k16(c, g, 1), k2 = k16(c, g, 2), k3 = k16(c, g, 3);
                    const size_t o = (((size_t)l * 16 + cb) * 16 + c) * 64 + lane;
                    wf16[o] = make_float4(Wl[j * Wd + k0], Wl[j * Wd + k1], Wl[j * Wd + k2], Wl[j * Wd + k3]);
                    wb16[o] = make_float4(Wl[k0 * Wd + j], Wl[k1 * Wd + j], Wl[k2 * Wd + j], Wl[k3 * Wd + j]);
                }
    }
    // backward pack for the 4-row-group GEMM (v_mfma_f32_4x4x1, gemm4 of mfma_gemm.h): the gradient at a layer's inputs is
    // sum_k G[row][k] W[k][j] (W [out = k][in = j]); lane l of column block cb holds W[4 kq .. 4 kq + 3][64 cb + l]
    // (and the forward pack of the same GEMM, pass2_body_g4: sum_k H[row][k] W[j][k], lane l of block cb holds W[64 cb + l][k0 .. k3])
    std::vector<float4>&wb4 = pk.wb4, &wf4 = pk.wf4;
    wb4.assign((size_t)std::max(nhh, 1) * 4 * 64 * 64, make_float4(0, 0, 0, 0));
    wf4.assign(wb4.size(), make_float4(0, 0, 0, 0));
    for (int l = 0; l < nhh; ++l) {
        const float* Wl = W[l + 1];
        for (int cb = 0; cb < 4; ++cb)
            for (int kq = 0; kq < 64; ++kq)
                for (int lane = 0; lane < 64; ++lane) {
                    const int j = 64 * cb + lane, s0 = 4 * kq;   // positions 4 kq .. +3 of the gradient tile
                    const int k0 = omds_kat(s0), k1 = omds_kat(s0 + 1), k2 = omds_kat(s0 + 2), k3 = omds_kat(s0 + 3);
                    wb4[(((size_t)l * 4 + cb) * 64 + kq) * 64 + lane] =
                        make_float4(Wl[(size_t)k0 * Wd + j], Wl[(size_t)k1 * Wd + j], Wl[(size_t)k2 * Wd + j], Wl[(size_t)k3 * Wd + j]);
                    wf4[(((size_t)l * 4 + cb) * 64 + kq) * 64 + lane] =
                        make_float4(Wl[(size_t)j * Wd + k0], Wl[(size_t)j * Wd + k1], Wl[(size_t)j * Wd + k2], Wl[(size_t)j * Wd + k3]);
                }
    }
    // last layer: 16x16x4 B-fragments, channels padded to 16
    const float* WL = W[n_linear - 1];
    std::vector<float4>& wl = pk.wl;
    wl.assign(16 * 64, make_float4(0, 0, 0, 0));
    for (int c = 0; c < 16; ++c)
        for (int lane = 0; lane < 64; ++lane) {
            const int j = lane & 15;   // the last layer reads the tile like gemm16 (load_a16): the same ascending k sequence
            float v[4] = {0, 0, 0, 0};
            if (j < C)
                for (int mm = 0; mm < 4; ++mm) v[mm] = WL[j * Wd + k16(c, lane >> 4, mm)];
            wl[c * 64 + lane] = make_float4(v[0], v[1], v[2], v[3]);
        }
    pk.bl.assign(OMDS_CPAD, 0.f);
    pk.wlraw.assign((size_t)C * Wd, 0.f);
    std::memcpy(pk.bl.data(), b[n_linear - 1], C * sizeof(float));
    std::memcpy(pk.wlraw.data(), WL, (size_t)C * Wd * sizeof(float));
    // first layer: transposed copy + backward pack over the 3d features (padded to 32 columns)
    const int F = 3 * d;
    pk.w1t.assign((size_t)F * Wd, 0.f);
    pk.b1.assign(Wd, 0.f);
    for (int c = 0; c < Wd; ++c)
        for (int f = 0; f < F; ++f) pk.w1t[(size_t)f * Wd + c] = W[0][c * F + f];
    std::memcpy(pk.b1.data(), b[0], Wd * sizeof(float));
    std::vector<float4>& w1b = pk.w1b;
    w1b.assign(32 * 64, make_float4(0, 0, 0, 0));
    for (int c = 0; c < 32; ++c)
        for (int lane = 0; lane < 64; ++lane) {
            const int f = lane & 31, s0 = 8 * c + 4 * (lane >> 5);
            float v[4] = {0, 0, 0, 0};
            if (f < F)
                for (int mm = 0; mm < 4; ++mm) v[mm] = W[0][omds_kat(s0 + mm) * F + f];
            w1b[c * 64 + lane] = make_float4(v[0], v[1], v[2], v[3]);
        }
    std::vector<float4>& w1b16 = pk.w1b16;
    w1b16.assign(16 * 2 * 64, make_float4(0, 0, 0, 0));
    for (int c = 0; c < 16; ++c)
        for (int jb = 0; jb < 2; ++jb)
            for (int lane = 0; lane < 64; ++lane) {
                const int f = 16 * jb + (lane & 15), g = lane >> 4;
                float v[4] = {0, 0, 0, 0};
                if (f < F)
                    for (int mm = 0; mm < 4; ++mm) v[mm] = W[0][k16(c, g, mm) * F + f];
                w1b16[(c * 2 + jb) * 64 + lane] = make_float4(v[0], v[1], v[2], v[3]);
            }
    // first layer, forward: K = 32 over the encoded inputs at positions 0..31 of the tile rows (feature omds_kat(position), zero
    // weights for the padding 3d .. 31), in the fragment orders of gemm_k32 and gemm16_k32
    std::vector<float4>& w1f = pk.w1f;
    w1f.assign(OMDS_NCB * 4 * 64, make_float4(0, 0, 0, 0));
    for (int cb = 0; cb < OMDS_NCB; ++cb)
        for (int c = 0; c < 4; ++c)
            for (int lane = 0; lane < 64; ++lane) {
                const int j = 32 * cb + (lane & 31), s0 = 8 * c + 4 * (lane >> 5);
                float v[4];
                for (int mm = 0; mm < 4; ++mm) { const int kk = omds_kat(s0 + mm); v[mm] = kk < F ? W[0][(size_t)j * F + kk] : 0.f; }
                w1f[((size_t)cb * 4 + c) * 64 + lane] = make_float4(v[0], v[1], v[2], v[3]);
            }
    std::vector<float4>& w1f16 = pk.w1f16;
    w1f16.assign(16 * 2 * 64, make_float4(0, 0, 0, 0));
    for (int cb = 0; cb < 16; ++cb)
        for (int c = 0; c < 2; ++c)
            for (int lane = 0; lane < 64; ++lane) {
                const int j = 16 * cb + (lane & 15), g = lane >> 4;
                float v[4];
                for (int mm = 0; mm < 4; ++mm) { const int kk = k16(c, g, mm); v[mm] = kk < F ? W[0][(size_t)j * F + kk] : 0.f; }
                w1f16[((size_t)cb * 2 + c) * 64 + lane] = make_float4(v[0], v[1], v[2], v[3]);
            }
    pk.whraw.assign((size_t)std::max(nhh, 1) * Wd * Wd, 0.f);
    for (int l = 0; l < nhh; ++l) std::memcpy(&pk.whraw[(size_t)l * Wd * Wd], W[l + 1], (size_t)Wd * Wd * sizeof(float));
    if ((act == OMDS_ACT_RELU || act == OMDS_ACT_TANH) && nhh >= 1 && nhh <= 4) {
        // the padded fp32 weights stay on the host: the screening pack is built again when the unit order changes (screen_reorder)
        pk.host_W.assign(Wpad.begin(), Wpad.end());
        pk.host_b.assign(bpad.begin(), bpad.end());
        pk.out_dims.assign(out_dims, out_dims + n_linear);
        build_screen_pack(pk, nullptr);
    }
    // transposed copies for the per-tile compaction (pass1_tile_dyn): row k = the weights leaving unit k
    pk.wht.assign((size_t)std::max(nhh, 1) * Wd * Wd, 0.f);
    for (int l = 0; l < nhh; ++l)
        for (int j = 0; j < Wd; ++j)
            for (int kk = 0; kk < Wd; ++kk) pk.wht[((size_t)l * Wd + kk) * Wd + j] = W[l + 1][(size_t)j * Wd + kk];
    pk.wlt.assign((size_t)Wd * 16, 0.f);
    for (int j = 0; j < C; ++j)
        for (int kk = 0; kk < Wd; ++kk) pk.wlt[(size_t)kk * 16 + j] = WL[(size_t)j * Wd + kk];
    pk.f_fwd = 0.0;
    for (int i = 0; i < n_linear; ++i) pk.f_fwd += 2.0 * in_dims[i] * out_dims[i];   // algorithmic: un-padded
    pk.f_bwd = pk.f_fwd - 2.0 * in_dims[n_linear - 1] * out_dims[n_linear - 1];   // no weight-gradient, no last-layer GEMM
    return OMDS_OK;
}
#undef PREQ

#ifdef OMDS_TEST_HOOKS
// Test hook (include/omds_test.h): the host half of omds_set_mlp_ex alone -- validation, padding, every fragment pack -- with no
// device and no context, so that the sanitizer build can run it on the CPU.  *checksum = FNV-1a over all packs in upload order
// (the screening pack, then MlpPacks::for_each_pack), *bytes = their total size; message of a failure through omds_last_error(NULL).
int omds_test_pack_mlp(int n_dof, int n_linear, const int32_t* in_dims, const int32_t* out_dims, const float* const* W,
                       const float* const* b, int act, float out_div, int n_skips, const int32_t* skip_after, uint64_t* checksum,
                       int64_t* bytes) {
    MlpPacks pk;
    const int rc = build_mlp_packs(n_dof, n_linear, in_dims, out_dims, W, b, act, out_div, n_skips, skip_after, pk, g_create_err);
    if (rc) return rc;
    uint64_t h = 1469598103934665603ull;
    int64_t total = 0;
    auto mix = [&](const void* p, size_t nb) {
        const unsigned char* c = static_cast<const unsigned char*>(p);
        for (size_t i = 0; i < nb; ++i) { h ^= c[i]; h *= 1099511628211ull; }
        total += (int64_t)nb;
    };
    mix(pk.wh.data(), pk.wh.size() * 2); mix(pk.sbias.data(), pk.sbias.size() * 4);
    pk.for_each_pack([&](const auto& v, auto) { mix(v.data(), v.size() * sizeof(v[0])); return 0; });
    // the screening pack once more in another unit order (what screen_reorder does behind a calibration): every hidden level reversed.
    // A permuted pack holds the same multiset of weights per slice row set; its bytes go into the same checksum
    if (!pk.host_W.empty() && pk.skip_mask == 0) {
        std::vector<int32_t> order((size_t)(pk.nhh + 1) * OMDS_WIDTH);
        for (int L = 0; L <= pk.nhh; ++L)
            for (int q = 0; q < OMDS_WIDTH; ++q) order[(size_t)L * OMDS_WIDTH + q] = OMDS_WIDTH - 1 - q;
        build_screen_pack(pk, order.data());
        mix(pk.wh.data(), pk.wh.size() * 2); mix(pk.sbias.data(), pk.sbias.size() * 4);
    }
    if (checksum) *checksum = h;
    if (bytes) *bytes = total;
    return OMDS_OK;
}
#endif
