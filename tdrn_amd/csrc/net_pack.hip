// net_pack.hip -- weight packing of a plan (net_plan.h): BatchNorm folding, OIHW -> [Cout][tap][Cin], into the host image of
// the caller-owned weight blob.
#include <cmath>
#include <cstring>

#include "net_plan.h"

namespace tdrn {

unsigned short host_f32_to_bf16(float f)
{
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (unsigned short)((u >> 16) | 0x40);   // NaN
    return (unsigned short)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
unsigned short host_f32_to_f16(float f)
{
    _Float16 h = (_Float16)f;
    unsigned short r;
    memcpy(&r, &h, 2);
    return r;
}

namespace {

struct Packer {
    const Plan &p;
    const StagedParams &staged;
    char *host;

    const std::vector<float> *get(const std::string &name) const
    {
        auto it = staged.find(name);
        return it == staged.end() ? nullptr : &it->second;
    }
    void put_elem(char *dst, size_t idx, float v) const
    {
        if (p.cfg.dtype == TDRN_F32) ((float *)dst)[idx] = v;
        else if (p.cfg.dtype == TDRN_BF16) ((unsigned short *)dst)[idx] = host_f32_to_bf16(v);
        else ((unsigned short *)dst)[idx] = host_f32_to_f16(v);
    }
    // y = scale*conv + shift  with BatchNorm (eps 1e-5, running stats) folded in double
    int fold(const Op &o, int Cout, std::vector<double> &scale, std::vector<double> &shift) const
    {
        scale.assign(Cout, 1.0);
        shift.assign(Cout, 0.0);
        if (!o.b.empty() && o.kind != OP_DEFORM) {
            const auto *b = get(o.b + ".bias");
            if (!b) return TDRN_E_PARAM;
            for (int c = 0; c < Cout; ++c) shift[c] = (*b)[c];
        }
        if (!o.bn.empty()) {
            const auto *g = get(o.bn + ".weight"), *be = get(o.bn + ".bias"), *mu = get(o.bn + ".running_mean"),
                       *var = get(o.bn + ".running_var");
            if (!g || !be || !mu || !var) return TDRN_E_PARAM;
            for (int c = 0; c < Cout; ++c) {
                const double s = (double)(*g)[c] / std::sqrt((double)(*var)[c] + 1e-5);
                scale[c] = s;
                shift[c] = (shift[c] - (double)(*mu)[c]) * s + (double)(*be)[c];
            }
        }
        return TDRN_OK;
    }

    int pack_first(const Op &o) const
    {
        const auto *w = get(o.w + ".weight");
        if (!w) return TDRN_E_PARAM;
        std::vector<double> sc, sh;
        TDRN_TRY(fold(o, o.Cout, sc, sh));
        float *dw = (float *)(host + o.w_off), *db = (float *)(host + o.b_off);
        for (int c = 0; c < o.Cout; ++c) {
            for (int k = 0; k < 27; ++k) dw[c * 27 + k] = (float)((double)(*w)[(size_t)c * 27 + k] * sc[c]);
            db[c] = (float)sh[c];
        }
        return TDRN_OK;
    }

    // ConvTranspose2d weight (Cin, Cout, 2, 2): slab(i,j)[co][ci] = W[ci][co][i][j]
    int pack_conv_transpose(const Op &o, const std::vector<float> &w) const
    {
        const int Creal = p.tensors[o.in].C;
        const int Cout = (int)p.params[p.param_index.at(o.w + ".weight")].shape[1];
        char *dw = host + o.w_off;
        float *db = (float *)(host + o.b_off);
        for (int ph = 0; ph < 4; ++ph)
            for (int co = 0; co < Cout; ++co)
                for (int ci = 0; ci < Creal; ++ci)
                    put_elem(dw, ((size_t)ph * o.Npad + co) * o.Cin + ci, w[(((size_t)ci * Cout + co) * 2 + (ph >> 1)) * 2 + (ph & 1)]);
        if (!o.b.empty()) {
            const auto *b = get(o.b + ".bias");
            if (!b) return TDRN_E_PARAM;
            for (int co = 0; co < Cout; ++co) db[co] = (*b)[co];
        }
        return TDRN_OK;
    }

    int pack_conv(const Op &o) const
    {
        const auto *w = get(o.w + ".weight");
        if (!w) return TDRN_E_PARAM;
        if (o.phases == 4) return pack_conv_transpose(o, *w);
        const int Creal = p.tensors[o.in].C, Cin = o.Cin, k = o.k, taps = k * k;
        char *dw = host + o.w_off;
        float *db = (float *)(host + o.b_off);
        const int Cout = (int)p.params[p.param_index.at(o.w + ".weight")].shape[0];
        std::vector<double> sc, sh;
        TDRN_TRY(fold(o, Cout, sc, sh));
        for (int co = 0; co < Cout; ++co) {
            for (int t = 0; t < taps; ++t)
                for (int ci = 0; ci < Creal; ++ci)
                    put_elem(dw, ((size_t)co * taps + t) * Cin + ci, (float)((double)(*w)[((size_t)co * Creal + ci) * taps + t] * sc[co]));
            db[co] = (float)sh[co];
        }
        if (o.w2.empty()) return TDRN_OK;
        // merge a centred k2 x k2 conv (same stride/dilation) into the k x k taps
        const auto *w2 = get(o.w2 + ".weight");
        if (!w2) return TDRN_E_PARAM;
        const int k2 = o.k2, d = (k - k2) / 2;
        std::vector<float> merged((size_t)Cout * taps * Creal, 0.f);
        for (int co = 0; co < Cout; ++co)
            for (int ci = 0; ci < Creal; ++ci) {
                for (int t = 0; t < taps; ++t)
                    merged[((size_t)co * taps + t) * Creal + ci] = (*w)[((size_t)co * Creal + ci) * taps + t];
                for (int r = 0; r < k2; ++r)
                    for (int q = 0; q < k2; ++q)
                        merged[((size_t)co * taps + (r + d) * k + (q + d)) * Creal + ci] += (*w2)[((size_t)co * Creal + ci) * k2 * k2 + r * k2 + q];
            }
        for (int co = 0; co < Cout; ++co)
            for (int t = 0; t < taps; ++t)
                for (int ci = 0; ci < Creal; ++ci)
                    put_elem(dw, ((size_t)co * taps + t) * Cin + ci, merged[((size_t)co * taps + t) * Creal + ci]);
        if (!o.b2.empty()) {
            const auto *b2 = get(o.b2 + ".bias");
            if (!b2) return TDRN_E_PARAM;
            for (int co = 0; co < Cout; ++co) db[co] += (*b2)[co];
        }
        return TDRN_OK;
    }

    int pack_l2norm(const Op &o) const
    {
        const auto *w = get(o.w + ".weight");
        if (!w) return TDRN_E_PARAM;
        memcpy(host + o.w_off, w->data(), w->size() * 4);
        return TDRN_OK;
    }

    int pack_dw(const Op &o) const
    {
        const auto *w = get(o.w + ".weight");
        if (!w) return TDRN_E_PARAM;
        const Tensor &ti = p.tensors[o.in];
        std::vector<double> sc, sh;
        TDRN_TRY(fold(o, ti.C, sc, sh));
        float *dw = (float *)(host + o.w_off), *db = (float *)(host + o.b_off);
        for (int c = 0; c < ti.C; ++c) {
            for (int t = 0; t < 9; ++t) dw[(size_t)t * ti.Cpad + c] = (float)((double)(*w)[(size_t)c * 9 + t] * sc[c]);
            db[c] = (float)sh[c];
        }
        return TDRN_OK;
    }

    int pack_offset(const Op &o) const
    {
        float *dw = (float *)(host + o.w_off), *db = (float *)(host + o.b_off);
        const std::string *names[2] = {&o.w, &o.w2};
        const std::string *bnames[2] = {&o.b, &o.b2};
        int row = 0;
        for (int i = 0; i < 2; ++i) {
            if (names[i]->empty()) continue;
            const auto *w = get(*names[i] + ".weight");
            if (!w) return TDRN_E_PARAM;
            const int n = (int)(w->size() / 12);
            memcpy(dw + (size_t)row * 12, w->data(), w->size() * 4);
            if (!bnames[i]->empty()) {
                const auto *b = get(*bnames[i] + ".bias");
                if (!b) return TDRN_E_PARAM;
                memcpy(db + row, b->data(), b->size() * 4);
            }
            row += n;
        }
        return TDRN_OK;
    }

    // [loc ; conf] rows of the heads of one pyramid level: per branch [Cout][tap][Cin] for the gather kernel, and for the
    // transform-then-sample plans the rows (tap, column) of the 1x1 GEMM: tap-major over the branches, 80 columns per tap,
    // three taps per 256-row slice (deform_y_col)
    int pack_deform(const Op &o) const
    {
        const int C = p.tensors[o.in].C;
        int tap0 = 0;
        for (int br = 0; br < o.n_branches; ++br) {
            const std::string &ln = br ? o.w2 : o.w, &cn = br ? o.b2 : o.b;
            const auto *wl = get(ln + ".weight"), *wc = get(cn + ".weight");
            if (!wl || !wc) return TDRN_E_PARAM;
            const int k = br ? o.k2 : o.k, taps = k * k;
            char *dw = host + (br ? o.w2_off : o.w_off), *dt = host + o.wt_off;
            for (int co = 0; co < o.Cout; ++co) {
                const std::vector<float> &src = co < 12 ? *wl : *wc;
                const int cs = co < 12 ? co : co - 12;
                for (int t = 0; t < taps; ++t)
                    for (int ci = 0; ci < C; ++ci) {
                        const float v = src[((size_t)cs * C + ci) * taps + t];
                        put_elem(dw, ((size_t)co * taps + t) * o.Cin + ci, v);
                        if (o.y_t >= 0) put_elem(dt, ((size_t)(co / 80) * o.y_cols + deform_y_col(tap0 + t) + co % 80) * o.Cin + ci, v);
                    }
            }
            tap0 += taps;
        }
        return TDRN_OK;
    }
};

}  // namespace

int pack_weights(const Plan &p, const StagedParams &staged, std::vector<char> &host)
{
    host.assign(p.blob_bytes, 0);
    const Packer pk{p, staged, host.data()};
    for (const Op &o : p.ops)
        switch (o.kind) {
            case OP_FIRST: TDRN_TRY(pk.pack_first(o)); break;
            case OP_CONV: TDRN_TRY(pk.pack_conv(o)); break;
            case OP_L2NORM: TDRN_TRY(pk.pack_l2norm(o)); break;
            case OP_DW: TDRN_TRY(pk.pack_dw(o)); break;
            case OP_OFFSET: TDRN_TRY(pk.pack_offset(o)); break;
            case OP_DEFORM: TDRN_TRY(pk.pack_deform(o)); break;
            default: break;
        }
    return TDRN_OK;
}

}  // namespace tdrn
