// Host side of libdmme_hip: the UNet execution plan (layer graph, parameter table,
// packed-weight layout, workspace layout, launch sequence) and the extern "C" API.
#include "plan.h"

#include <functional>
#include <map>
#include <mutex>

namespace dmme {

static thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int debug_route(const char* key, int dflt) {
    const char* e = getenv("DMME_DEBUG_ROUTE");
    if (!e || !*e) return dflt;
    const size_t kl = strlen(key);
    for (const char* p = e; *p;) {
        const char* end = strchr(p, ',');
        const size_t len = end ? (size_t)(end - p) : strlen(p);
        if (len >= kl && !strncmp(p, key, kl) && (len == kl || p[kl] == '=')) return len == kl ? 1 : atoi(p + kl + 1);
        if (!end) break;
        p = end + 1;
    }
    return dflt;
}

}  // namespace dmme

using namespace dmme;

namespace dmme {

struct Node {
    int kind;  // 0 res, 1 down, 2 up
    std::string prefix;
    int cin, cout;
    bool attn;
    // parameter indices
    int gn1w = -1, gn1b = -1, c1w = -1, c1b = -1, tw = -1, tb = -1, gn2w = -1, gn2b = -1, c2w = -1, c2b = -1;
    int rw = -1, rb = -1, anw = -1, anb = -1, qw = -1, qb = -1, pw = -1, pb = -1;
    int cw = -1, cb = -1;  // down / up conv
    int tproj_col = 0;
};

struct Builder {
    dmme_plan* P;
    int64_t ref_cursor = 0;

    int add_param(const std::string& name, std::initializer_list<int64_t> shape, bool is_buffer, bool as_f32,
                  int cout, int cin, int taps) {
        Param p;
        p.name = name;
        p.ndim = (int)shape.size();
        int i = 0;
        for (auto s : shape) p.shape[i++] = s;
        p.ref_off = ref_cursor;
        p.is_buffer = is_buffer;
        p.as_f32 = as_f32;
        p.cout = cout;
        p.cin = cin;
        p.taps = taps;
        ref_cursor += p.numel();
        P->params.push_back(p);
        return (int)P->params.size() - 1;
    }
    void conv(const std::string& p, int ci, int co, int k, int& w, int& b) {
        w = add_param(p + ".weight", {co, ci, k, k}, false, false, co, ci, k * k);
        b = add_param(p + ".bias", {co}, false, true, 1, co, 1);
    }
    void lin(const std::string& p, int ci, int co, int& w, int& b) {
        w = add_param(p + ".weight", {co, ci}, false, false, co, ci, 1);
        b = add_param(p + ".bias", {co}, false, true, 1, co, 1);
    }
    void gn(const std::string& p, int c, int& w, int& b) {
        w = add_param(p + ".weight", {c}, false, true, 1, c, 1);
        b = add_param(p + ".bias", {c}, false, true, 1, c, 1);
    }
    void res_params(Node& n) {
        const dmme_unet_cfg& c = P->cfg;
        const std::string& p = n.prefix;
        if (c.arch == DMME_ARCH_IDDPM) {
            // iddpm.ResBlock.__init__ registration order (models/iddpm.py:85-104): conv1 (built with p = 0: conv at index 2),
            // norm, condition (Linear emb -> 2 c_out), conv2 = norm_act_drop_conv(...)[1:] (the slice keeps the keys 1..3)
            gn(p + ".conv1.0", n.cin, n.gn1w, n.gn1b);
            conv(p + ".conv1.2", n.cin, n.cout, 3, n.c1w, n.c1b);
            gn(p + ".norm", n.cout, n.gn2w, n.gn2b);
            lin(p + ".condition.0", c.emb_dim, 2 * n.cout, n.tw, n.tb);
            conv(p + (c.dropout > 0 ? ".conv2.3" : ".conv2.2"), n.cout, n.cout, 3, n.c2w, n.c2b);
            if (n.cin != n.cout) conv(p + ".residual", n.cin, n.cout, 1, n.rw, n.rb);
            if (n.attn) {
                gn(p + ".attention.norm", n.cout, n.anw, n.anb);
                conv(p + ".attention.qkv_proj", n.cout, 3 * n.cout, 1, n.qw, n.qb);
                conv(p + ".attention.proj", n.cout, n.cout, 1, n.pw, n.pb);
            }
            return;
        }
        gn(p + ".conv1.0", n.cin, n.gn1w, n.gn1b);
        conv(p + ".conv1.2", n.cin, n.cout, 3, n.c1w, n.c1b);
        lin(p + ".condition.0", c.emb_dim, n.cout, n.tw, n.tb);
        gn(p + ".conv2.0", n.cout, n.gn2w, n.gn2b);
        // norm_act_drop_conv (models/ddpm.py:25-35): conv index 3 with Dropout2d, 2 without
        conv(p + (c.dropout > 0 ? ".conv2.3" : ".conv2.2"), n.cout, n.cout, 3, n.c2w, n.c2b);
        if (n.cin != n.cout) conv(p + ".residual", n.cin, n.cout, 1, n.rw, n.rb);
        if (n.attn) {
            gn(p + ".attention.norm", n.cout, n.anw, n.anb);
            conv(p + ".attention.qkv_proj", n.cout, 3 * n.cout, 1, n.qw, n.qb);
            conv(p + ".attention.proj", n.cout, n.cout, 1, n.pw, n.pb);
        }
    }
};

bool in_list(const int* v, int n, int x) {
    for (int i = 0; i < n; ++i)
        if (v[i] == x) return true;
    return false;
}

int build_plan(dmme_plan* P) {
    const dmme_unet_cfg& c = P->cfg;
    const int nb = c.num_blocks, nd = c.num_depths;
    const int B = P->B;
    const int64_t es = (int64_t)dtype_size(P->dtype);

    // ---- layer graph: UNet.__init__ (models/ddpm.py:203-279) ----
    std::vector<int> chans;
    chans.push_back(c.channels_per_depth[0]);
    for (int d = 0; d < nd; ++d)
        for (int b = 0; b < nb; ++b) chans.push_back(c.channels_per_depth[d]);
    const int L = (int)chans.size();  // len(channels)
    auto is_cut = [&](int layer_num) {  // layer_num in downsample_layers = {nb*i : 1 <= i < nd}
        return layer_num > 0 && layer_num % nb == 0 && layer_num / nb <= nd - 1;
    };
    auto has_attn = [&](int depth) { return in_list(c.attention_depths, c.num_attention_depths, depth); };

    std::vector<Node> down, mid, up;
    int depth = 1;
    for (int i = 0; i + 1 < L; ++i) {
        Node n{0, "down_layers." + std::to_string(down.size()), chans[i], chans[i + 1], has_attn(depth)};
        down.push_back(n);
        if (is_cut(i + 1)) {
            Node d{1, "down_layers." + std::to_string(down.size()), chans[i + 1], chans[i + 1], false};
            down.push_back(d);
            ++depth;
        }
    }
    // the reference's `if down_layers[-1] == len(channels) - 1` (:242) compares a module
    // with an int and is never true: the up path starts with ResBlocks, never an UpSample
    depth = nd;
    for (int i = 0; i + 1 < L; ++i) {
        const int ci = chans[L - 1 - i], co = chans[L - 2 - i];
        const bool at = has_attn(depth);
        const int layer_num = L - 1 - i;
        up.push_back(Node{0, "up_layers." + std::to_string(up.size()), 2 * ci, co, at});
        if (is_cut(layer_num - 1)) {
            up.push_back(Node{0, "up_layers." + std::to_string(up.size()), 2 * co, co, at});
            up.push_back(Node{2, "up_layers." + std::to_string(up.size()), co, co, false});
            --depth;
        }
    }
    up.push_back(Node{0, "up_layers." + std::to_string(up.size()), 2 * chans[0], chans[0], has_attn(1)});
    const int top = chans[L - 1];
    mid.push_back(Node{0, "middle_layers.0", top, top, true});
    mid.push_back(Node{0, "middle_layers.1", top, top, false});
    if (c.arch == DMME_ARCH_IDDPM)  // MultiHeadAttention asserts dim % num_heads == 0 (models/iddpm.py:26)
        for (auto* seq : {&down, &up, &mid})
            for (auto& n : *seq)
                DMME_REQUIRE(!n.attn || n.cout % c.num_heads == 0, DMME_ERR_INVALID, "%s: attention width %d not divisible by num_heads=%d",
                             n.prefix.c_str(), n.cout, c.num_heads);

    DMME_REQUIRE(!(P->mix && has_attn(1)), DMME_ERR_UNSUPPORTED, "precision fp16r32: attention at the full-resolution level (attention_depths contains 1) is not supported");

    // ---- parameter table in nn.Module registration order ----
    Builder bld{P};
    const int half = c.pos_dim / 2;
    P->freqs_param = bld.add_param("condition.0.embeddings", {1, half}, true, true, 1, half, 1);
    int l1w, l1b, l2w, l2b, icw, icb, ogw, ogb, ocw, ocb;
    bld.lin("condition.1", c.pos_dim, c.emb_dim, l1w, l1b);
    bld.lin("condition.3", c.emb_dim, c.emb_dim, l2w, l2b);
    P->p_l1w = l1w; P->p_l1b = l1b; P->p_l2w = l2w; P->p_l2b = l2b;
    bld.conv("input_conv", c.in_channels, chans[0], 3, icw, icb);
    const bool cls = c.arch == DMME_ARCH_CLASSIFIER;  // the encoder half + head: no up path, no output conv
    if (cls) up.clear();
    for (auto* seq : {&down, &up, &mid})
        for (auto& n : *seq) {
            if (n.kind == 0)
                bld.res_params(n);
            else if (n.kind == 1)
                bld.conv(n.prefix, n.cin, n.cout, 3, n.cw, n.cb);
            else
                bld.conv(n.prefix + ".conv", n.cin, n.cout, 3, n.cw, n.cb);
        }
    if (cls) {  // out = GroupNorm(C_top) -> SiLU -> mean over H x W -> Linear(C_top, num_classes); all four stay fp32 when packed
        const int top = chans[L - 1];
        bld.gn("out.0", top, P->p_hgw, P->p_hgb);
        P->p_hw = bld.add_param("out.2.weight", {c.num_classes, top}, false, true, c.num_classes, top, 1);
        P->p_hb = bld.add_param("out.2.bias", {c.num_classes}, false, true, 1, c.num_classes, 1);
        P->out_channels = c.num_classes;
        ogw = ogb = ocw = ocb = -1;
    } else {
        bld.gn("output_conv.0", chans[0], ogw, ogb);
        P->out_channels = c.arch == DMME_ARCH_IDDPM ? 2 * c.in_channels : c.in_channels;
        bld.conv("output_conv.2", chans[0], P->out_channels, 3, ocw, ocb);
    }
    if (P->cond)  // behind everything else: an unconditional flat buffer is a prefix of a conditional one.  Row num_classes: the null label
        P->p_lemb = bld.add_param("label_emb.weight", {c.num_classes + 1, c.emb_dim}, false, true, c.num_classes + 1, c.emb_dim, 1);
    P->ref_numel = bld.ref_cursor;

    // ---- packed layout: the per-block time projections form one [sumCout][emb] matrix ----
    int tcols = 0;
    for (auto* seq : {&down, &up, &mid})
        for (auto& n : *seq)
            if (n.kind == 0) {
                const int width = c.arch == DMME_ARCH_IDDPM ? 2 * n.cout : n.cout;  // (shift | scale) for the scale-shift blocks
                n.tproj_col = tcols;
                tcols += width;
                P->tblocks.push_back({n.tw, n.tb, n.tproj_col, width});
            }
    P->tproj_cols = tcols;
    auto layout_packed = [&]() {
        int64_t cur = 0;
        P->tproj_w_off = cur;
        cur = align_up(cur + (int64_t)tcols * c.emb_dim * es, 256);
        P->tproj_b_off = cur;
        cur = align_up(cur + (int64_t)tcols * 4, 256);
        std::unordered_map<int, const Node*> tw_owner, tb_owner;
        for (auto* seq : {&down, &up, &mid})
            for (auto& n : *seq)
                if (n.kind == 0) {
                    tw_owner[n.tw] = &n;
                    tb_owner[n.tb] = &n;
                }
        for (int i = 0; i < (int)P->params.size(); ++i) {
            Param& p = P->params[i];
            if (tw_owner.count(i)) {
                p.packed_off = P->tproj_w_off + (int64_t)tw_owner[i]->tproj_col * c.emb_dim * es;
            } else if (tb_owner.count(i)) {
                p.packed_off = P->tproj_b_off + (int64_t)tb_owner[i]->tproj_col * 4;
            } else {
                p.packed_off = cur;
                cur = align_up(cur + p.numel() * ((p.as_f32 || p.pack_code >= 3) ? 4 : es), 256);
            }
        }
        P->packed_bytes = cur;
    };
    {   // transposed + tap-flipped conv weights for the data-gradient convolutions
        int64_t bc = 0;
        for (Param& p : P->params)
            if (p.ndim == 4) {
                p.packed_bwd_off = bc;
                bc = align_up(bc + p.numel() * es, 256);
            }
        P->packed_bwd_bytes = bc;
    }

    // ---- workspace + op list ----
    int64_t ws = 0;
    auto ws_alloc = [&](int64_t bytes) {
        const int64_t o = ws;
        ws = align_up(ws + bytes, 256);
        return o;
    };
    auto is_top = [&](int H_, int W_) { return P->mix && H_ == P->H && W_ == P->W; };
    auto new_tensor = [&](int C, int H, int W, int force16 = 0) {
        Tensor t;
        t.C = C;
        t.H = H;
        t.W = W;
        t.f32 = is_top(H, W) && !force16;
        t.off = ws_alloc((int64_t)B * H * W * C * (t.f32 ? 4 : es));
        P->tensors.push_back(t);
        return (int)P->tensors.size() - 1;
    };
    P->ws_mark = ws_alloc(16);
    P->ws_tsin = ws_alloc((int64_t)B * c.pos_dim * 4);
    P->ws_th1 = ws_alloc((int64_t)B * c.emb_dim * 4);
    P->ws_temb = ws_alloc((int64_t)B * c.emb_dim * 4);
    P->ws_tz1 = ws_alloc((int64_t)B * c.emb_dim * 4);
    P->ws_tz2 = ws_alloc((int64_t)B * c.emb_dim * 4);
    P->ws_tproj = ws_alloc((int64_t)B * tcols * 4);

    std::vector<Op>& ops = P->ops;
    {
        Op o{};
        o.kind = OP_SINUS;
        ops.push_back(o);
        Op a{};
        a.kind = OP_LINEAR;
        a.lin_in = P->ws_tsin; a.lin_out = P->ws_th1; a.lin_K = c.pos_dim; a.lin_N = c.emb_dim;
        a.lin_pre = P->ws_tz1;
        a.lin_w = l1w; a.lin_b = l1b; a.lin_silu = 1;
        ops.push_back(a);
        Op b{};
        b.kind = OP_LINEAR;
        b.lin_in = P->ws_th1; b.lin_out = P->ws_temb; b.lin_K = c.emb_dim; b.lin_N = c.emb_dim;
        b.lin_pre = P->ws_tz2;
        b.lin_w = l2w; b.lin_b = l2b; b.lin_silu = 1;
        if (P->cond) {  // the pre-activation alone (the wave kernel of small batches writes no second output): the label op finishes the layer
            b.lin_out = P->ws_tz2;
            b.lin_pre = -1;
            b.lin_silu = 0;
        }
        ops.push_back(b);
        if (P->cond) {
            Op l{};
            l.kind = OP_LABEL;
            P->label_op = (int)ops.size();
            ops.push_back(l);
        }
        Op d{};
        d.kind = OP_LINEAR;  // all per-block projections at once (w/b = -1: concatenated region)
        d.lin_in = P->ws_temb; d.lin_out = P->ws_tproj; d.lin_K = c.emb_dim; d.lin_N = tcols;
        d.lin_w = -1; d.lin_b = -1; d.lin_silu = 0;
        ops.push_back(d);
    }
    size_t gn_part_max = 0;
    auto emit_gn = [&](int s1, int s2, int gw, int gb) {
        Op o{};
        o.kind = OP_GN;
        o.gn_src1 = s1; o.gn_src2 = s2; o.gn_gamma = gw; o.gn_beta = gb;
        const Tensor& t1 = P->tensors[s1];
        const int C = t1.C + (s2 >= 0 ? P->tensors[s2].C : 0);
        o.gn_scale = ws_alloc((int64_t)B * C * 4);
        o.gn_shift = ws_alloc((int64_t)B * C * 4);
        o.gn_mr = ws_alloc((int64_t)B * c.num_groups * 2 * 4);
        const size_t part = gn_fast_scratch_floats(B, t1.H * t1.W, C, c.num_groups);
        if (part > gn_part_max) gn_part_max = part;
        ops.push_back(o);
        return (int)ops.size() - 1;
    };
    int64_t dmask_cursor = 0;
    int cur_t, H = P->H, W = P->W;
    {
        Op o{};
        o.kind = OP_CONV;
        o.src1 = -2; o.w = icw; o.b = icb; o.taps = 9;
        o.dst = new_tensor(chans[0], H, W);
        if (P->mix) {  // fp32 in, fp32 out: the fp32 instance of the input conv (its 27-deep products are fp32 MFMAs anyway)
            o.route_f32 = 1;
            P->params[icw].pack_code = 3;
        }
        ops.push_back(o);
        cur_t = o.dst;
        P->named["input_conv"] = cur_t;
    }
    std::vector<int> skips{cur_t};

    auto emit_res = [&](const Node& n, int x1, int x2) {
        const Tensor tx = P->tensors[x1];
        const int h = tx.H, w = tx.W;
        const bool iddpm = P->cfg.arch == DMME_ARCH_IDDPM;
        const int g1 = emit_gn(x1, x2, n.gn1w, n.gn1b);
        Op c1{};
        c1.kind = OP_CONV;
        c1.src1 = x1; c1.src2 = x2; c1.w = n.c1w; c1.b = n.c1b; c1.gn = g1; c1.pro_silu = 1;
        c1.tproj_col = iddpm ? -1 : n.tproj_col; c1.taps = 9;  // DDPM: h += Linear(t_emb) in the epilogue (models/ddpm.py:129)
        c1.dst = new_tensor(n.cout, h, w);
        const bool top = is_top(h, w);
        if (top) {
            c1.mix = 1;
            P->params[n.c1w].pack_code = 4;
        }
        ops.push_back(c1);
        const int hmid = c1.dst;
        const int g2 = emit_gn(hmid, -1, n.gn2w, n.gn2b);
        if (iddpm) {  // h = norm(h) * (scale + 1) + shift (models/iddpm.py:117-118)
            ops[g2].gn_mod_col = n.tproj_col;
            ops[g2].gn_mod_C = n.cout;
        }
        int r1 = x1, r2 = x2;
        if (n.cin != n.cout) {
            Op rc{};
            rc.kind = OP_CONV;
            rc.src1 = x1; rc.src2 = x2; rc.w = n.rw; rc.b = n.rb; rc.taps = 1;
            rc.dst = new_tensor(n.cout, h, w);
            if (top) {
                rc.mix = 4;
                P->params[n.rw].pack_code = 4;
            }
            ops.push_back(rc);
            r1 = rc.dst;
            r2 = -1;
        }
        Op c2{};
        c2.kind = OP_CONV;
        c2.src1 = hmid; c2.w = n.c2w; c2.b = n.c2b; c2.gn = g2; c2.pro_silu = 1; c2.taps = 9;
        if (P->cfg.dropout > 0) c2.dmask_off = dmask_cursor;
        dmask_cursor += (int64_t)B * n.cout;
        c2.res1 = r1; c2.res2 = r2;
        c2.dst = new_tensor(n.cout, h, w);
        if (top) {
            c2.mix = 1;
            P->params[n.c2w].pack_code = 4;
        }
        ops.push_back(c2);
        int out = c2.dst;
        if (n.attn) {
            const int g3 = emit_gn(out, -1, n.anw, n.anb);
            Op q{};
            q.kind = OP_CONV;
            q.src1 = out; q.w = n.qw; q.b = n.qb; q.gn = g3; q.taps = 1;
            q.dst = new_tensor(3 * n.cout, h, w);
            ops.push_back(q);
            Op at{};
            at.kind = OP_ATTN;
            at.at_qkv = q.dst;
            at.at_heads = iddpm ? P->cfg.num_heads : 1;
            at.at_out = new_tensor(n.cout, h, w);
            at.at_lse = ws_alloc((int64_t)B * at.at_heads * h * w * 4);
            ops.push_back(at);
            Op pr{};
            pr.kind = OP_CONV;
            pr.src1 = at.at_out; pr.w = n.pw; pr.b = n.pb; pr.taps = 1; pr.res1 = out;
            pr.dst = new_tensor(n.cout, h, w);
            ops.push_back(pr);
            out = pr.dst;
        }
        P->named[n.prefix] = out;
        return out;
    };

    for (auto& n : down) {
        if (n.kind == 0) {
            cur_t = emit_res(n, cur_t, -1);
        } else {
            DMME_REQUIRE(H % 2 == 0 && W % 2 == 0, DMME_ERR_UNSUPPORTED, "odd resolution %dx%d at a DownSample", H, W);
            if (P->tensors[cur_t].f32) {  // leaving the fp32 level: the stride-2 conv reads a 16-bit copy
                Op cs{};
                cs.kind = OP_CAST;
                cs.cast_src = cur_t;
                cs.cast_dst = new_tensor(P->tensors[cur_t].C, H, W, 1);
                ops.push_back(cs);
                cur_t = cs.cast_dst;
            }
            Op o{};
            o.kind = OP_CONV;
            o.src1 = cur_t; o.w = n.cw; o.b = n.cb; o.taps = 9; o.stride = 2;
            H /= 2; W /= 2;
            o.dst = new_tensor(n.cout, H, W);
            ops.push_back(o);
            cur_t = o.dst;
            P->named[n.prefix] = cur_t;
        }
        skips.push_back(cur_t);
    }
    for (auto& n : mid) cur_t = emit_res(n, cur_t, -1);
    for (auto& n : up) {
        if (n.kind == 0) {
            DMME_REQUIRE(!skips.empty(), DMME_ERR_INVALID, "skip stack underflow");
            const int sk = skips.back();
            skips.pop_back();
            const Tensor &a = P->tensors[cur_t], &b = P->tensors[sk];
            DMME_REQUIRE(a.C + b.C == n.cin && a.H == b.H && a.W == b.W, DMME_ERR_INVALID,
                         "%s: concat %d+%d channels does not match conv input %d", n.prefix.c_str(), a.C, b.C, n.cin);
            cur_t = emit_res(n, cur_t, sk);  // torch.cat([x, skip]) : x first (:310)
        } else {
            Op o{};
            o.kind = OP_CONV;
            o.src1 = cur_t; o.w = n.cw; o.b = n.cb; o.taps = 9; o.up = 1;
            H *= 2; W *= 2;
            o.dst = new_tensor(n.cout, H, W);
            if (is_top(H, W)) {  // entering the fp32 level from the 16-bit one: split passes on a 16-bit source
                o.mix = P->tensors[cur_t].f32 ? 1 : 2;
                P->params[n.cw].pack_code = 4;
            }
            ops.push_back(o);
            cur_t = o.dst;
            P->named[n.prefix] = cur_t;
        }
    }
    if (cls) {
        P->head_src = cur_t;
    } else {
        const int g = emit_gn(cur_t, -1, ogw, ogb);
        Op o{};
        o.kind = OP_CONV;
        o.src1 = cur_t; o.w = ocw; o.b = ocb; o.gn = g; o.pro_silu = 1; o.taps = 9; o.dst = -2;
        if (P->mix && P->tensors[cur_t].f32) {
            o.mix = 3;
            P->params[ocw].pack_code = 4;
        }
        ops.push_back(o);
    }
    P->dropmask_numel = dmask_cursor;
    if (P->mix) {
        // which split-pass 3x3 convs run TWO passes: bit k of the mask = the k-th such conv in op order (default below; DMME_DEBUG_ROUTE
        // r32_2pass=<mask> overrides, r32_2pass=0 = three passes everywhere)
        const int mask = debug_route("r32_2pass", kR32TwoPassDefault);
        int k = 0;
        for (Op& o : ops)
            if (o.kind == OP_CONV && (o.mix == 1 || o.mix == 2)) {
                o.mix2 = (mask >> k) & 1;
                ++k;
            }
    }
    layout_packed();  // (after the op list: a mixed plan's convs choose their filter layouts above)
    P->ws_gnpart = ws_alloc((int64_t)(gn_part_max ? gn_part_max : 1) * 4);
    {   // up to 4 partial images of the widest small-map conv (either direction: its data gradient has Cin outputs)
        int64_t mx = 0;
        for (const Op& o : ops) {
            if (o.kind != OP_CONV || o.taps != 9 || o.src1 < 0 || o.dst < 0) continue;
            const Tensor &ti = P->tensors[o.src1], &to = P->tensors[o.dst];
            if (to.H * to.W > 64 || o.stride != 1 || o.up) continue;
            const int cin = ti.C + (o.src2 >= 0 ? P->tensors[o.src2].C : 0);
            const int64_t v = (int64_t)B * to.H * to.W * (cin > to.C ? cin : to.C);
            if (v > mx) mx = v;
        }
        P->splitk_floats = 4 * mx;
        P->ws_splitk = ws_alloc(P->splitk_floats * 4 + 16);
    }
    P->ws_bytes = ws;
    P->n_launches = (int)ops.size();

    return DMME_OK;
}

// re-pack items: (cout range) x (cin range) sub-blocks of at most 8192 elements (the LDS tile of pack_table_kernel).
// wide_co: prefer long cout runs (the transposed data-gradient layout writes runs of couts), else long cin runs.
static void push_pack_items(const Param& p, int64_t dst_off, int as_f32, bool wide_co, std::vector<PackItem>& items) {
    const int LIMIT = 8192;
    int nco, nci;
    if (as_f32 == 1) {
        nci = p.cin;
        nco = LIMIT / (p.cin * p.taps);
        if (nco < 1) nco = 1;
    } else if (wide_co) {
        nco = p.cout < 64 ? p.cout : 64;
        nci = LIMIT / (nco * p.taps);
        if (nci > p.cin) nci = p.cin;
        if (nci >= 4) nci &= ~3;  // whole 16-byte vectors per source run (pack_table_kernel's vector loads)
        if (nci < 1) nci = 1;
    } else {
        nci = p.cin;
        if (nci * p.taps > LIMIT) nci = LIMIT / p.taps;
        nco = LIMIT / (nci * p.taps);
        if (nco < 1) nco = 1;
    }
    if (as_f32 != 1 && nco > 256) nco = 256;  // the odd LDS pitch adds one float per cout: keep that within the tile's slack
    for (int r0 = 0; r0 < p.cout; r0 += nco)
        for (int c0 = 0; c0 < p.cin; c0 += nci) {
            PackItem it;
            it.src_off = p.ref_off;
            it.dst_off = dst_off;
            it.cout = p.cout;
            it.cin = p.cin;
            it.taps = p.taps;
            it.row0 = r0;
            it.rows = p.cout - r0 < nco ? p.cout - r0 : nco;
            it.ci0 = c0;
            it.nci = p.cin - c0 < nci ? p.cin - c0 : nci;
            it.as_f32 = as_f32;
            items.push_back(it);
        }
}

void build_pack_items(const dmme_plan* P, std::vector<PackItem>& items) {
    for (const Param& p : P->params) push_pack_items(p, p.packed_off, p.pack_code >= 0 ? p.pack_code : p.as_f32 ? 1 : 0, false, items);
}

void build_pack_items_bwd(const dmme_plan* P, std::vector<PackItem>& items) {
    for (const Param& p : P->params)
        if (p.packed_bwd_off >= 0) push_pack_items(p, p.packed_bwd_off, 2, true, items);
}

void build_unpack_items(const dmme_plan* P, std::vector<PackItem>& items) {
    const int64_t CHUNK = 16384;
    for (const Param& p : P->params) {
        if (p.wp_off < 0) continue;
        const int64_t row = (int64_t)p.cin * p.taps;
        int64_t rows_per = CHUNK / row;
        if (rows_per < 1) rows_per = 1;
        for (int64_t r0 = 0; r0 < p.cout; r0 += rows_per) {
            PackItem it;
            it.src_off = p.ref_off;  // destination: reference-layout gradient (float offset)
            it.dst_off = p.wp_off;   // source: packed-layout image (float offset)
            it.cout = p.cout;
            it.cin = p.cin;
            it.taps = p.taps;
            it.row0 = (int32_t)r0;
            it.rows = (int32_t)((p.cout - r0) < rows_per ? (p.cout - r0) : rows_per);
            it.ci0 = 0;
            it.nci = p.cin;
            it.as_f32 = 0;
            items.push_back(it);
        }
    }
}

// fill the device-side descriptor of a conv op
// fwd: the forward launch (a conv whose GroupNorm pre-activated its input reads that tensor and applies nothing); the backward
// passes false and sees the raw sources with their scale / shift / mask, which is what it differentiates through
void fill_conv(const dmme_plan* P, const Op& o, const char* packed, const float* x, float* y, char* ws,
               const float* drop_masks, int nt, ConvArgs& a, bool fwd) {
    const int64_t es = (int64_t)dtype_size(P->dtype);
    (void)es;
    a.x3 = P->x3 || o.route_f32;
    a.f16 = P->dtype == DMME_F16 && !o.route_f32;
    a.mix = o.mix;
    a.mix2 = o.mix2;
    a.N = P->B;
    if (o.src1 == -2) {
        a.src1 = x;
        a.in_nchw = 1;
        a.C1 = P->cfg.in_channels;
        a.Hin = P->H;
        a.Win = P->W;
    } else {
        const Tensor& t = P->tensors[o.src1];
        a.src1 = ws + t.off;
        a.C1 = t.C;
        a.Hin = t.H;
        a.Win = t.W;
    }
    if (o.src2 >= 0) {
        a.src2 = ws + P->tensors[o.src2].off;
        a.C2 = P->tensors[o.src2].C;
    }
    const Param& w = P->params[o.w];
    a.w = packed + w.packed_off;
    a.bias = (const float*)(packed + P->params[o.b].packed_off);
    a.Cout = w.cout;
    a.taps = o.taps;
    a.stride = o.stride;
    a.up = o.up;
    const int Hv = o.up ? 2 * a.Hin : a.Hin, Wv = o.up ? 2 * a.Win : a.Win;
    a.Hout = Hv / o.stride;
    a.Wout = Wv / o.stride;
    if (o.gn >= 0) {
        a.scale = (const float*)(ws + P->ops[o.gn].gn_scale);
        a.shift = (const float*)(ws + P->ops[o.gn].gn_shift);
        const Op& g = P->ops[o.gn];
        if (fwd && g.gn_in_consumer) {
            const Tensor& t1 = P->tensors[g.gn_src1];
            const Tensor* t2 = g.gn_src2 >= 0 ? &P->tensors[g.gn_src2] : nullptr;
            a.has_gni = 1;
            a.gni.p1 = (const float*)(ws + t1.stats_off);
            a.gni.t1 = t1.stats_tiles;
            a.gni.cnt1 = t1.stats_cnt;
            a.gni.C1 = t1.C;
            a.gni.p2 = t2 ? (const float*)(ws + t2->stats_off) : nullptr;
            a.gni.t2 = t2 ? t2->stats_tiles : 0;
            a.gni.cnt2 = t2 ? t2->stats_cnt : 0;
            a.gni.C2 = t2 ? t2->C : 0;
            a.gni.groups = P->cfg.num_groups;
            a.gni.gamma = (const float*)(packed + P->params[g.gn_gamma].packed_off);
            a.gni.beta = (const float*)(packed + P->params[g.gn_beta].packed_off);
            a.gni.eps = 1e-5f;
            a.gni.mean_rstd = (float*)(ws + g.gn_mr);
            if (g.gn_mod_col >= 0) {  // scale-shift conditioning: (shift | scale) columns of the batched time projection
                a.gni.t_shift = (const float*)(ws + P->ws_tproj) + g.gn_mod_col;
                a.gni.t_scale = a.gni.t_shift + g.gn_mod_C;
                a.gni.t_ld = P->tproj_cols;
                a.gni.nt = nt;
            }
        }
    }
    a.pro_silu = o.pro_silu;
    a.out_silu = o.out_silu;
    if (o.dmask_off >= 0 && drop_masks) a.dmask = drop_masks + o.dmask_off;
    if (fwd && o.use_act) {
        a.src1 = ws + P->ops[o.gn].gn_act;
        a.C1 = a.C1 + a.C2;
        a.src2 = nullptr;
        a.C2 = 0;
        a.scale = a.shift = a.dmask = nullptr;
        a.pro_silu = 0;
    }
    if (o.tproj_col >= 0) {
        a.tproj = (const float*)(ws + P->ws_tproj) + o.tproj_col;
        a.tproj_ld = P->tproj_cols;
        a.nt = nt;
    }
    if (fwd && o.rseg >= 0) {  // the block's residual conv runs inside this launch: no residual tensor
        const Op& rc = P->ops[o.rseg];
        const Tensor& r1 = P->tensors[rc.src1];
        a.r_src1 = ws + r1.off;
        a.r_C1 = r1.C;
        if (rc.src2 >= 0) {
            a.r_src2 = ws + P->tensors[rc.src2].off;
            a.r_C2 = P->tensors[rc.src2].C;
        }
        a.r_w = packed + P->params[rc.w].packed_off;
        a.r_bias = (const float*)(packed + P->params[rc.b].packed_off);
    } else if (o.res1 >= 0) {
        a.res1 = ws + P->tensors[o.res1].off;
        a.R1 = P->tensors[o.res1].C;
        if (o.res2 >= 0) a.res2 = ws + P->tensors[o.res2].off;
    }
    if (P->splitk_floats > 0 && ws) {
        a.splitk = (float*)(ws + P->ws_splitk);
        a.splitk_cap = P->splitk_floats;
    }
    if (fwd && o.gd_n > 0) {
        a.n_gno = o.gd_n;
        a.gn_eps = 1e-5f;
        a.gn_cg = P->tensors[o.dst].C / P->cfg.num_groups;
        for (int k = 0; k < o.gd_n; ++k) {
            const Op& g = P->ops[o.gd_gn[k]];
            GnOut& G = a.gno[k];
            G.gamma = (const float*)(packed + P->params[g.gn_gamma].packed_off);
            G.beta = (const float*)(packed + P->params[g.gn_beta].packed_off);
            G.scale = (float*)(ws + g.gn_scale);
            G.shift = (float*)(ws + g.gn_shift);
            G.mean_rstd = (float*)(ws + g.gn_mr);
            G.C = P->tensors[g.gn_src1].C + (g.gn_src2 >= 0 ? P->tensors[g.gn_src2].C : 0);
            G.cg = G.C / P->cfg.num_groups;
            G.c_off = o.gd_coff[k];
            if (k == o.gd_act) {
                const Op& cv = P->ops[g.gn_consumer];
                a.act = ws + g.gn_act;
                a.act_k = k;
                a.act_silu = cv.pro_silu;
                a.act_dmask = (cv.dmask_off >= 0 && drop_masks) ? drop_masks + cv.dmask_off : nullptr;
            }
        }
    }
    a.gn_raw_moments = P->mix ? 1 : 0;
    if (o.dst == -2) {
        a.dst = y;
        a.out_nchw = 1;
    } else {
        const Tensor& td = P->tensors[o.dst];
        a.dst = ws + td.off;
        if (td.stats_off >= 0) {
            a.gn_part = (float*)(ws + td.stats_off);
            a.gn_cg = td.C / P->cfg.num_groups;
            a.gn_tiles = td.stats_tiles;
        }
    }
}

// can this GroupNorm be finalised from the partials its producers emitted?
bool gn_from_parts(const dmme_plan* P, const Op& o) {
    if (o.gn_force_small) return false;
    const Tensor& t1 = P->tensors[o.gn_src1];
    if (t1.stats_off < 0) return false;
    const int G = P->cfg.num_groups;
    int C = t1.C;
    if (o.gn_src2 >= 0) {
        const Tensor& t2 = P->tensors[o.gn_src2];
        if (t2.stats_off < 0) return false;
        C += t2.C;
        const int cg = C / G;
        if (t1.C % cg || cg % (t1.C / G) || cg % (t2.C / G)) return false;
    }
    return true;
}

// decide which conv outputs carry fused GroupNorm partials (needs the launch-time tile choice) and give them room
void assign_stats(dmme_plan* P) {
    std::vector<char> wanted(P->tensors.size(), 0);
    for (const Op& o : P->ops)
        if (o.kind == OP_GN && o.lvl < 0) {  // (norms inside a level run are finished by the engine)
            wanted[o.gn_src1] = 1;
            if (o.gn_src2 >= 0) wanted[o.gn_src2] = 1;
        }
    const int G = P->cfg.num_groups;
    int64_t ws = P->ws_bytes;
    for (const Op& o : P->ops) {
        if (o.kind != OP_CONV || o.dst < 0 || !wanted[o.dst] || o.lvl >= 0) continue;
        Tensor& td = P->tensors[o.dst];
        if (td.C % G) continue;
        ConvArgs a{};
        fill_conv(P, o, (const char*)4096, (const float*)4096, (float*)4096, (char*)4096, nullptr, 1, a);
        a.nt = o.tproj_col >= 0 ? P->B : 0;  // training adds one time-embedding row per image
        int tiles = 0, px = 0;
        if (!conv_stats_query(conv_dt(P, o), a, td.C / G, &tiles, &px)) continue;
        td.stats_tiles = tiles;
        td.stats_cnt = px * (td.C / G);
        td.stats_off = ws;
        ws = align_up(ws + (int64_t)P->B * tiles * G * 2 * 4, 256);
    }
    P->ws_bytes = ws;
}

// Small maps again, from the producer's side: a conv whose tile is 64 pixels of WHOLE images (8x8, 4x4 maps) sees every value of an
// (image, group) in one workgroup, so its epilogue can finish the norms that consume its output - scale / shift / {mean, rstd} rows
// and, for a single-source norm, the consumer's pre-activated input - and the norm itself is no launch at all
// (conv_epilogue_store_direct).  A tensor goes this way only if ALL the norms reading it do (else it would need partials as well),
// and a norm only if all its sources do.
void assign_direct(dmme_plan* P) {
    const int nT = (int)P->tensors.size(), nO = (int)P->ops.size();
    const int G = P->cfg.num_groups;
    std::vector<int> producer(nT, -1);
    for (int oi = 0; oi < nO; ++oi)
        if (P->ops[oi].kind == OP_CONV && P->ops[oi].dst >= 0 && P->ops[oi].lvl < 0) producer[P->ops[oi].dst] = oi;
    struct Use { int gn, coff; };
    std::vector<std::vector<Use>> uses(nT);
    for (int oi = 0; oi < nO; ++oi) {
        const Op& g = P->ops[oi];
        if (g.kind != OP_GN || g.lvl >= 0) continue;
        uses[g.gn_src1].push_back({oi, 0});
        if (g.gn_src2 >= 0) uses[g.gn_src2].push_back({oi, P->tensors[g.gn_src1].C});
    }
    std::vector<char> elig(nT, 0);
    for (int t = 0; t < nT; ++t) {
        if (producer[t] < 0 || uses[t].empty() || uses[t].size() > 2) continue;
        const Op& o = P->ops[producer[t]];
        ConvArgs a{};
        fill_conv(P, o, (const char*)4096, (const float*)4096, (float*)4096, (char*)4096, nullptr, 1, a);
        a.nt = o.tproj_col >= 0 ? P->B : 0;
        a.gn_part = nullptr;
        a.n_gno = (int)uses[t].size();
        bool ok = true;
        int cgs[2] = {0, 0};
        for (size_t k = 0; k < uses[t].size(); ++k) {
            const Op& g = P->ops[uses[t][k].gn];
            const int C = P->tensors[g.gn_src1].C + (g.gn_src2 >= 0 ? P->tensors[g.gn_src2].C : 0);
            if (g.gn_mod_col >= 0 || C % G || uses[t][k].coff % (C / G)) ok = false;
            cgs[k] = C / G;
        }
        a.gn_cg = P->tensors[t].C / G;
        if (ok) elig[t] = (char)conv_gn_direct_query(conv_dt(P, o), a, cgs, (int)uses[t].size());
        if (elig[t] == 2 && P->tensors[t].C % G) elig[t] = 0;  // (2: no act output)
    }
    for (bool changed = true; changed;) {  // a norm needs all its sources, a tensor all its norms
        changed = false;
        for (int t = 0; t < nT; ++t) {
            if (!elig[t]) continue;
            for (const Use& u : uses[t]) {
                const Op& g = P->ops[u.gn];
                if (!elig[g.gn_src1] || (g.gn_src2 >= 0 && !elig[g.gn_src2])) {
                    elig[t] = 0;
                    changed = true;
                    break;
                }
            }
        }
    }
    int64_t ws = P->ws_bytes;
    const int64_t es = (int64_t)dtype_size(P->dtype);
    for (int t = 0; t < nT; ++t) {
        if (!elig[t]) continue;
        Op& o = P->ops[producer[t]];
        P->tensors[t].stats_off = -1;  // no partials: nothing merges them
        o.gd_n = (int)uses[t].size();
        for (int k = 0; k < o.gd_n; ++k) {
            o.gd_gn[k] = uses[t][k].gn;
            o.gd_coff[k] = uses[t][k].coff;
            P->ops[uses[t][k].gn].gn_direct = 1;
        }
    }
    if (getenv("DMME_NO_PREACT")) return;
    // single-source direct norms: the producer also writes the consumer's pre-activated input
    for (int ci = 0; ci < nO; ++ci) {
        Op& cv = P->ops[ci];
        if (cv.kind != OP_CONV || cv.gn < 0 || cv.src1 < 0 || cv.up || cv.stride != 1 || cv.lvl >= 0) continue;
        Op& g = P->ops[cv.gn];
        if (!g.gn_direct || g.gn_src2 >= 0 || g.gn_act >= 0 || g.gn_src1 != cv.src1 || cv.src2 >= 0) continue;
        Op& pr = P->ops[producer[g.gn_src1]];
        if (pr.gd_act >= 0 || elig[g.gn_src1] != 1) continue;  // one pre-activated output per producer; not from the two-pass kernel
        for (int k = 0; k < pr.gd_n; ++k)
            if (pr.gd_gn[k] == cv.gn) pr.gd_act = k;
        if (pr.gd_act < 0) continue;
        const Tensor& t1 = P->tensors[g.gn_src1];
        g.gn_act = ws;
        g.gn_consumer = ci;
        cv.use_act = 1;
        ws = align_up(ws + (int64_t)P->B * t1.H * t1.W * t1.C * es, 256);
    }
    P->ws_bytes = ws;
}

// Small maps: the GroupNorms that run as one workgroup per image (maps of at most 64 pixels: their producers tile several images
// together and cannot fuse the statistics) also write the consumer conv's pre-activated input, once per element.  Not for the
// scale-shift blocks of the IDDPM UNet (their per-(n, c) affine is modulated after the norm kernel).
void assign_preact(dmme_plan* P) {
    int64_t ws = P->ws_bytes;
    const int64_t es = (int64_t)dtype_size(P->dtype);
    for (int ci = 0; ci < (int)P->ops.size(); ++ci) {
        Op& cv = P->ops[ci];
        if (cv.kind != OP_CONV || cv.gn < 0 || cv.src1 < 0 || cv.up || cv.stride != 1 || cv.lvl >= 0) continue;
        Op& g = P->ops[cv.gn];
        constexpr bool over_parts = false;  // (the whole-image norm kernel over tensors whose producers left partials: measured neutral, below)
        if (g.gn_mod_col >= 0 || g.gn_act >= 0 || g.gn_direct) continue;
        const Tensor& t1 = P->tensors[g.gn_src1];
        const int C2 = g.gn_src2 >= 0 ? P->tensors[g.gn_src2].C : 0;
        if (g.gn_src1 != cv.src1 || g.gn_src2 != cv.src2) continue;
        if (!gn_small_act_supported(P->dtype, t1.H * t1.W, t1.C, C2, P->cfg.num_groups)) continue;
        // 8x8 maps: one image per 64-pixel tile, so the producers did leave partials and the norm is a 5 us finalize launch.  Taking
        // the whole-image kernel there instead (DMME_PREACT_PARTS=1) was measured neutral: the consumers drop 34.9 -> 29.1 us, the
        // three-pass norm kernel costs 12 us instead of 5.5 (step 2.999 vs 3.016 ms) - off by default
        if (gn_from_parts(P, g)) {
            if (!over_parts) continue;
            g.gn_force_small = 1;
        }
        g.gn_act = ws;
        g.gn_consumer = ci;
        cv.use_act = 1;
        ws = align_up(ws + (int64_t)P->B * t1.H * t1.W * (t1.C + C2) * es, 256);
    }
    P->ws_bytes = ws;
}

// GroupNorm statistics folded with the affine into per-(n, c) scale / shift for the consuming conv's prologue
// Norms finished by their CONSUMER: a conv on the wave-specialised kernel whose norm's statistics are the producers' partials merges
// them in its parameter fill (ws_fill_par_gni) - no finalize launch between the two convolutions.
void assign_gn_in(dmme_plan* P) {
    for (Op& cv : P->ops) {
        if (cv.kind != OP_CONV || cv.gn < 0 || cv.use_act || cv.lvl >= 0) continue;
        Op& g = P->ops[cv.gn];
        if (g.gn_direct || g.gn_in_consumer || g.gn_act >= 0 || !gn_from_parts(P, g)) continue;
        if (g.gn_src1 != cv.src1 || g.gn_src2 != cv.src2) continue;
        const Tensor& t1 = P->tensors[g.gn_src1];
        // partials per consumer group: tiles x (producer groups per consumer group), at most 64 (one or two batches of loads in the
        // fill); 64x64 maps have hundreds - the batched finalize kernel's job
        const int G = P->cfg.num_groups, Cn = t1.C + (g.gn_src2 >= 0 ? P->tensors[g.gn_src2].C : 0);
        bool fits = t1.stats_tiles * ((Cn / G) / (t1.C / G)) <= 64;
        if (g.gn_src2 >= 0) {
            const Tensor& t2 = P->tensors[g.gn_src2];
            fits = fits && t2.stats_tiles * ((Cn / G) / (t2.C / G)) <= 64;
        }
        if (!fits) continue;
        ConvArgs a{};
        fill_conv(P, cv, (const char*)4096, (const float*)4096, (float*)4096, (char*)4096, nullptr, 1, a);
        a.nt = cv.tproj_col >= 0 ? P->B : 0;
        if (!conv_gn_in_query(conv_dt(P, cv), a)) continue;
        g.gn_in_consumer = 1;
    }
}

// The ResBlocks' 1x1 residual convs (models/ddpm.py:108-111: `h + residual(x)` where the channel count changes) whose conv2 runs on the
// wave-specialised 3x3 kernel's 256-pixel form become a second K segment of that launch (conv_pipe.hip, RSEG): at the benchmark batch the
// seven of them on the 32x32 / 16x16 levels were 0.17 ms of launches that mostly moved bytes (raw input in, residual tensor out, and
// in again in conv2's epilogue).  Forward only: the backward pass never reads a residual tensor.  DMME_DEBUG_ROUTE=no_rseg: off.
void assign_rseg(dmme_plan* P) {
    if (debug_route("no_rseg") || !is16(P->dtype) || P->mix || P->x3) return;
    std::vector<int> uses(P->tensors.size(), 0), producer(P->tensors.size(), -1);
    for (int oi = 0; oi < (int)P->ops.size(); ++oi) {
        const Op& o = P->ops[oi];
        for (int id : {o.src1, o.src2, o.res1, o.res2, o.gn_src1, o.gn_src2, o.at_qkv, o.cast_src})
            if (id >= 0) ++uses[id];
        if (o.kind == OP_CONV && o.dst >= 0) producer[o.dst] = oi;
    }
    for (int ci = 0; ci < (int)P->ops.size(); ++ci) {
        Op& c2 = P->ops[ci];
        if (c2.kind != OP_CONV || c2.taps != 9 || c2.lvl >= 0 || c2.res1 < 0 || c2.res2 >= 0 || c2.dst < 0 || c2.mix || c2.route_f32) continue;
        const int ri = producer[c2.res1];
        if (ri < 0 || uses[c2.res1] != 1) continue;
        Op& rc = P->ops[ri];
        if (rc.kind != OP_CONV || rc.taps != 1 || rc.lvl >= 0 || rc.gn >= 0 || rc.pro_silu || rc.out_silu || rc.dmask_off >= 0 || rc.tproj_col >= 0 || rc.res1 >= 0 ||
            rc.up || rc.stride != 1 || rc.src1 < 0 || rc.gd_n > 0 || rc.mix || rc.route_f32)
            continue;
        for (const auto& kv : P->named)  // (a tensor somebody can ask for by module name stays a tensor)
            if (kv.second == c2.res1) goto next;
        {
            c2.rseg = ri;
            ConvArgs a{};
            fill_conv(P, c2, (const char*)4096, (const float*)4096, (float*)4096, (char*)4096, nullptr, 1, a, true);
            if (!conv_route(P->dtype, a).rseg) {
                c2.rseg = -1;
                continue;
            }
            rc.fused_away = 1;
        }
    next:;
    }
}

// The attention blocks of the 16x16 maps (models/ddpm.py:66-75: `x + proj(attention(norm(x)))`): where the whole-row attention kernel
// serves the block (256 keys, single head, a launch that fills the chip), its proj 1x1 conv, bias, residual add and the next norm's
// partial statistics run inside that launch (attn_mfma.hip, AttnProj) - at the benchmark batch five launches of 8-15 us and the context
// tensor's round trip.  Forward only.  DMME_DEBUG_ROUTE=no_attn_proj: off.
void assign_attn_proj(dmme_plan* P) {
    if (P->x3) return;
    for (int ai = 0; ai + 1 < (int)P->ops.size(); ++ai) {
        Op& at = P->ops[ai];
        if (at.kind != OP_ATTN || at.lvl >= 0 || at.at_heads != 1) continue;
        Op& pr = P->ops[ai + 1];
        if (pr.kind != OP_CONV || pr.src1 != at.at_out || pr.src2 >= 0 || pr.taps != 1 || pr.lvl >= 0 || pr.gn >= 0 || pr.pro_silu || pr.out_silu || pr.dmask_off >= 0 ||
            pr.tproj_col >= 0 || pr.res1 < 0 || pr.res2 >= 0 || pr.up || pr.stride != 1 || pr.gd_n > 0 || pr.mix || pr.route_f32 || pr.dst < 0 || pr.fused_away || pr.rseg >= 0)
            continue;
        const Tensor &q = P->tensors[at.at_qkv], &td = P->tensors[pr.dst];
        if (q.f32 || td.f32 || P->tensors[pr.res1].f32 || P->tensors[at.at_out].f32) continue;
        const int S = q.H * q.W, C = q.C / 3;
        if (td.C != C || P->tensors[pr.res1].C != C) continue;
        const bool stats = td.stats_off >= 0;
        if (!attn_proj_fusable(P->dtype, P->B, S, C, stats ? td.C / P->cfg.num_groups : 0, stats ? td.stats_tiles : 0)) continue;
        at.at_proj = ai + 1;
        pr.fused_away = 2;
    }
}

// The no-grad form of those blocks (attn_mfma.hip, AttnFold): no qkv conv, no qkv tensor - the attention launch reads the block's raw input,
// finishes the norm from its producers' partials and uses matrices folded from the weights (dmme_unet_pack_folded: slots behind the
// packed parameters).  A block qualifies when its proj conv already rides in the launch, the qkv conv reads ONE tensor through a norm its
// consumer finishes from partials - or whose (scale, shift) rows are in the workspace by then: a norm its producers' epilogues finish, a
// norm with a launch - (no conditioning, no activation, no mask), nothing but the attention reads qkv, and the residual is that same tensor.
// DMME_NO_ATTN_FOLD: off (DMME_NO_ATTN_PROJ / DMME_NO_ATTN_FULL leave nothing to fold).  The backward-capable walk never folds.
void assign_attn_fold(dmme_plan* P) {
    if (getenv("DMME_NO_ATTN_FOLD") || debug_route("no_attn_fold") || !is16(P->dtype) || P->x3 || P->mix) return;
    int64_t cur = P->packed_bytes;
    const int64_t es = (int64_t)dtype_size(P->dtype);
    for (int ai = 1; ai < (int)P->ops.size(); ++ai) {
        Op& at = P->ops[ai];
        if (at.kind != OP_ATTN || at.at_proj < 0 || at.at_heads != 1 || at.lvl >= 0) continue;
        Op& qc = P->ops[ai - 1];
        const Op& pr = P->ops[at.at_proj];
        if (qc.kind != OP_CONV || qc.dst != at.at_qkv || qc.taps != 1 || qc.src1 < 0 || qc.src2 >= 0 || qc.gn < 0 || qc.pro_silu || qc.out_silu || qc.dmask_off >= 0 ||
            qc.tproj_col >= 0 || qc.res1 >= 0 || qc.res2 >= 0 || qc.up || qc.stride != 1 || qc.gd_n > 0 || qc.mix || qc.route_f32 || qc.fused_away || qc.rseg >= 0 ||
            qc.use_act || qc.lvl >= 0 || pr.res1 != qc.src1)
            continue;
        const Op& gn = P->ops[qc.gn];
        const Tensor& tx = P->tensors[qc.src1];
        const int C = tx.C, groups = P->cfg.num_groups;
        if (gn.kind != OP_GN || gn.gn_src1 != qc.src1 || gn.gn_src2 >= 0 || gn.gn_mod_col >= 0 || gn.gn_act >= 0 || tx.f32 ||
            (gn.gn_in_consumer && (tx.stats_off < 0 || tx.stats_tiles > 32)) || P->tensors[at.at_qkv].C != 3 * C || P->params[qc.w].pack_code >= 0 || P->params[pr.w].pack_code >= 0)
            continue;
        bool only_here = true;  // qkv read by nothing but this attention (forward ops; the backward reads it, and never follows a folded walk)
        for (int oi = 0; oi < (int)P->ops.size() && only_here; ++oi) {
            const Op& o = P->ops[oi];
            if (oi == ai) continue;
            if (o.kind == OP_CONV && (o.src1 == at.at_qkv || o.src2 == at.at_qkv || o.res1 == at.at_qkv || o.res2 == at.at_qkv)) only_here = false;
            if (o.kind == OP_GN && (o.gn_src1 == at.at_qkv || o.gn_src2 == at.at_qkv)) only_here = false;
            if (o.kind == OP_ATTN && o.at_qkv == at.at_qkv) only_here = false;
            if (o.kind == OP_CAST && o.cast_src == at.at_qkv) only_here = false;
        }
        const Tensor& td = P->tensors[pr.dst];
        const bool stats = td.stats_off >= 0;
        if (!only_here || !attn_fold_shape_ok(P->dtype, P->B, tx.H * tx.W, C, stats ? C / groups : 0, stats ? td.stats_tiles : 0)) continue;
        at.at_fold_qkv = ai - 1;
        qc.folded_into = ai;
        at.fold_M = cur;
        cur = align_up(cur + (int64_t)C * C * es, 256);
        at.fold_wpv = cur;
        cur = align_up(cur + (int64_t)C * C * es, 256);
        at.fold_c = cur;
        cur = align_up(cur + (int64_t)C * 4, 256);
        at.fold_b2 = cur;
        cur = align_up(cur + (int64_t)C * 4, 256);
        AttnFoldJob jb{};
        jb.wq = P->params[qc.w].packed_off;
        jb.bq = P->params[qc.b].packed_off;
        jb.wp = P->params[pr.w].packed_off;
        jb.bp = P->params[pr.b].packed_off;
        jb.M = at.fold_M;
        jb.c = at.fold_c;
        jb.wpv = at.fold_wpv;
        jb.bias2 = at.fold_b2;
        jb.C = C;
        P->fold_jobs.push_back(jb);
        if (C > P->fold_maxC) P->fold_maxC = C;
    }
    P->packed_bytes = cur;
}

int run_gn(const dmme_plan* P, const Op& o, const char* pk, char* ws, int nt, const float* drop_masks, hipStream_t s) {
    if (o.gn_direct || o.gn_in_consumer) return DMME_OK;  // its producers (its consumer) wrote scale / shift / {mean, rstd} (and act)
    // scale-shift conditioning (iddpm.ResBlock): (shift | scale) columns of the batched time projection
    const float* tsh = o.gn_mod_col >= 0 ? (const float*)(ws + P->ws_tproj) + o.gn_mod_col : nullptr;
    const float* tsc = tsh ? tsh + o.gn_mod_C : nullptr;
    int rc;
    const Tensor& t1 = P->tensors[o.gn_src1];
    const void* s1 = ws + t1.off;
    const void* s2 = o.gn_src2 >= 0 ? ws + P->tensors[o.gn_src2].off : nullptr;
    const int C2 = o.gn_src2 >= 0 ? P->tensors[o.gn_src2].C : 0;
    const float* gam = (const float*)(pk + P->params[o.gn_gamma].packed_off);
    const float* bet = (const float*)(pk + P->params[o.gn_beta].packed_off);
    float* sc = (float*)(ws + o.gn_scale);
    float* sh = (float*)(ws + o.gn_shift);
    if (gn_from_parts(P, o)) {
        const Tensor* t2 = o.gn_src2 >= 0 ? &P->tensors[o.gn_src2] : nullptr;
        return launch_gn_finalize_parts((const float*)(ws + t1.stats_off), t1.stats_tiles, t1.stats_cnt, t1.C,
                                        t2 ? (const float*)(ws + t2->stats_off) : nullptr, t2 ? t2->stats_tiles : 0,
                                        t2 ? t2->stats_cnt : 0, C2, P->B, P->cfg.num_groups, gam, bet, 1e-5f, sc, sh,
                                        (float*)(ws + o.gn_mr), tsh, tsc, P->tproj_cols, nt, s);
    }
    const int gdt = t1.f32 ? DMME_F32 : P->dtype;  // (a mixed plan's fp32 level; concatenated sources share a level)
    if (gn_fast_supported(gdt, P->B, t1.H * t1.W, t1.C, C2, P->cfg.num_groups)) {
        void* act = nullptr;
        int act_silu = 0;
        const float* dm = nullptr;
        if (o.gn_act >= 0) {
            const Op& cv = P->ops[o.gn_consumer];
            act = ws + o.gn_act;
            act_silu = cv.pro_silu;
            if (cv.dmask_off >= 0 && drop_masks) dm = drop_masks + cv.dmask_off;
        }
        rc = launch_gn_fast(gdt, s1, s2, P->B, t1.H * t1.W, t1.C, C2, P->cfg.num_groups, gam, bet, 1e-5f, sc, sh,
                            (float*)(ws + o.gn_mr), (float*)(ws + P->ws_gnpart), s, act, act_silu, dm);
    }
    else
        rc = launch_gn_generic(gdt, s1, s2, P->B, t1.H * t1.W, t1.C, C2, P->cfg.num_groups, gam, bet, 1e-5f, sc, sh,
                               (float*)(ws + o.gn_mr), s);
    if (rc != DMME_OK || !tsh) return rc;
    return launch_gn_modulate(sc, sh, tsh, tsc, P->tproj_cols, nt, P->B, o.gn_mod_C, s);
}

// keep_ctx: a backward pass may follow this forward (tensors only the backward reads are written: the fused attention block's context)
int run_op(const dmme_plan* P, const Op& o, const char* pk, const float* x, const int64_t* t, int nt, float* y,
           char* ws, const float* drop_masks, hipStream_t s, bool keep_ctx, const int64_t* labels = nullptr, int* status = nullptr) {
    if (o.lvl >= 0) return o.lvl_first ? run_level(P, P->lvl_runs[o.lvl], pk, ws, nt, drop_masks, s, keep_ctx) : DMME_OK;
    if (o.fused_away) return DMME_OK;  // a residual 1x1 conv that runs inside its block's conv2 (assign_rseg)
    // folded attention blocks: only where no backward follows AND this buffer's folded slots are current (never stale matrices)
    const bool fold = !keep_ctx && P->fold_packed == (const void*)pk;
    if (fold && o.kind == OP_CONV && o.folded_into >= 0) return DMME_OK;  // the qkv conv of a block that runs folded
    switch (o.kind) {
        case OP_SINUS:
            return launch_time_sinusoid(t, nt, (const float*)(pk + P->params[P->freqs_param].packed_off),
                                        P->cfg.pos_dim / 2, (float*)(ws + P->ws_tsin), s, (unsigned*)(ws + P->ws_mark),
                                        keep_ctx ? kFwdMarkKeep : kFwdMarkNograd);
        case OP_LINEAR: {
            const char* w = o.lin_w >= 0 ? pk + P->params[o.lin_w].packed_off : pk + P->tproj_w_off;
            const float* b = (const float*)(o.lin_b >= 0 ? pk + P->params[o.lin_b].packed_off : pk + P->tproj_b_off);
            if (nt > 4)
                return launch_small_gemm(P->dtype, 0, (const float*)(ws + o.lin_in), o.lin_K, w, o.lin_K, nt, o.lin_N, o.lin_K, b, o.lin_silu,
                                         (float*)(ws + o.lin_out), o.lin_N, s, o.lin_pre >= 0 ? (float*)(ws + o.lin_pre) : nullptr);
            return launch_linear_wave(P->dtype, (const float*)(ws + o.lin_in), nt, o.lin_K, w, b, o.lin_N, o.lin_silu,
                                      (float*)(ws + o.lin_out), s);
        }
        case OP_LABEL: {  // nt: the rows the time MLP ran with; writes B rows (and keeps z2 + E[y] for the backward where they are B too)
            float* z2 = (float*)(ws + P->ws_tz2);
            return launch_label_cond(z2, nt, (const float*)(pk + P->params[P->p_lemb].packed_off), labels, P->B, P->cfg.num_classes, P->cfg.emb_dim,
                                     (float*)(ws + P->ws_temb), nt == P->B ? z2 : nullptr, status, s);
        }
        case OP_GN:
            return run_gn(P, o, pk, ws, nt, drop_masks, s);
        case OP_CONV: {
            ConvArgs a{};
            fill_conv(P, o, pk, x, y, ws, drop_masks, nt, a, true);
            return launch_conv(conv_dt(P, o), a, s);
        }
        case OP_CAST: {
            const Tensor& ts = P->tensors[o.cast_src];
            return launch_cast_f32_to_16(P->dtype, (const float*)(ws + ts.off), (int64_t)P->B * ts.H * ts.W * ts.C, ws + P->tensors[o.cast_dst].off, s);
        }
        case OP_ATTN: {
            const Tensor& q = P->tensors[o.at_qkv];
            const int S = q.H * q.W, C = q.C / 3;
            if (fold && o.at_fold_qkv >= 0) {  // no qkv: the block's raw input, the norm's partials, the folded slots (assign_attn_fold)
                ConvArgs a{}, qa{};
                fill_conv(P, P->ops[o.at_proj], pk, x, y, ws, drop_masks, nt, a, true);
                fill_conv(P, P->ops[o.at_fold_qkv], pk, x, y, ws, drop_masks, nt, qa, true);
                return launch_attn_fold(P->dtype, qa.src1, P->B, S, C, qa.has_gni ? &qa.gni : nullptr, qa.scale, qa.shift, pk + o.fold_M, (const float*)(pk + o.fold_c), pk + o.fold_wpv,
                                        (const float*)(pk + o.fold_b2), a.res1, a.dst, a.gn_part, a.gn_tiles, a.gn_cg, s);
            }
            if (o.at_proj >= 0) {  // the block's proj conv + residual inside the launch (assign_attn_proj)
                ConvArgs a{};
                fill_conv(P, P->ops[o.at_proj], pk, x, y, ws, drop_masks, nt, a, true);
                return launch_attn_proj(P->dtype, ws + q.off, P->B, S, C, keep_ctx ? ws + P->tensors[o.at_out].off : nullptr, (float*)(ws + o.at_lse), a.w, a.bias,
                                        a.res1, a.dst, a.gn_part, a.gn_tiles, a.gn_cg, s);
            }
            if (P->x3 && attn_x3_supported(P->B, S, C, o.at_heads))  // (no log-sum-exp kept: the fp32 backward recomputes the scores)
                return launch_attn_x3(ws + q.off, P->B, S, C, o.at_heads, ws + P->tensors[o.at_out].off, s);
            if (o.at_heads > 1) {
                if (attn_heads_mfma_supported(P->dtype, P->B, S, C, o.at_heads))
                    return launch_attn_heads_mfma(P->dtype, ws + q.off, P->B, S, C, o.at_heads, ws + P->tensors[o.at_out].off, (float*)(ws + o.at_lse), s);
                return launch_attn_heads(P->dtype, ws + q.off, P->B, S, C, o.at_heads, ws + P->tensors[o.at_out].off, s);
            }
            if (attn_mfma_supported(P->dtype, P->B, S, C))
                return launch_attn_mfma(P->dtype, ws + q.off, P->B, S, C, ws + P->tensors[o.at_out].off, (float*)(ws + o.at_lse), s);
            return launch_attn_generic(P->dtype, ws + q.off, P->B, S, C, ws + P->tensors[o.at_out].off, s);
        }
    }
    return DMME_OK;
}
// kernel label + algorithmic flops / bytes of one op (bench.py's roofline accounting)
void op_account(const dmme_plan* P, const Op& o, char* label, int cap, double* flops, double* bytes) {
    const double es = (double)dtype_size(P->dtype);
    const char* tn = P->dtype == DMME_BF16 ? "bf16" : P->dtype == DMME_F16 ? "f16" : "float";  // (the conv labels add ":bf16x3" themselves)
    const double B = P->B;
    *flops = 0;
    *bytes = 0;
    if (o.lvl >= 0) {  // one launch for the whole run: accounted on its first op
        const LvlRun& R = P->lvl_runs[o.lvl];
        if (o.lvl_first) {
            snprintf(label, cap, "lvl_engine_kernel<%dx%d>", 1 << R.sh, 1 << R.sh);
            *flops = R.flops;
            *bytes = R.bytes;
        } else {
            snprintf(label, cap, "(level engine)");
        }
        return;
    }
    if (o.fused_away) {
        snprintf(label, cap, o.fused_away == 2 ? "(proj 1x1 conv inside its block's attention launch)" : "(residual 1x1 conv inside its block's conv2)");
        return;
    }
    switch (o.kind) {
        case OP_SINUS:
            snprintf(label, cap, "time_sinusoid_kernel");
            break;
        case OP_LABEL:
            snprintf(label, cap, "label_cond_kernel");
            *flops = B * P->cfg.emb_dim;
            *bytes = 4.0 * B * P->cfg.emb_dim * 3;
            break;
        case OP_LINEAR:
            snprintf(label, cap, "linear_wave_kernel<%s>", tn);
            *flops = 2.0 * o.lin_K * o.lin_N;  // one timestep row when sampling
            *bytes = (double)o.lin_K * o.lin_N * es + 4.0 * (o.lin_K + 2.0 * o.lin_N);
            break;
        case OP_GN: {
            const Tensor& t1 = P->tensors[o.gn_src1];
            const int C = t1.C + (o.gn_src2 >= 0 ? P->tensors[o.gn_src2].C : 0);
            const bool fast = gn_fast_supported(P->dtype, P->B, t1.H * t1.W, t1.C, C - t1.C, P->cfg.num_groups);
            if (o.gn_direct || o.gn_in_consumer) {  // no launch: "(...)" labels are skipped by the per-kernel tables
                snprintf(label, cap, o.gn_direct ? "(norm finished by its producers' epilogues)" : "(norm finished by its consumer's parameter fill)");
            } else if (gn_from_parts(P, o)) {
                snprintf(label, cap, "gn_finalize_parts_kernel");
                *bytes = 2.0 * B * C * 4;
            } else {
                snprintf(label, cap, fast ? "gn_partial_kernel<%s>" : "gn_generic_kernel<%s>", tn);
                *bytes = B * t1.H * t1.W * C * es + 2.0 * B * C * 4;
            }
            break;
        }
        case OP_CONV: {
            ConvArgs a{};
            fill_conv(P, o, (const char*)4096, (const float*)4096, (float*)4096, (char*)4096, nullptr, 1, a, true);
            const int cdt = conv_dt(P, o);
            conv_label(conv_route(cdt, a), cdt, a, label, cap);
            const double Cin = a.C1 + a.C2, opix = B * a.Hout * a.Wout;
            *flops = 2.0 * opix * a.Cout * Cin * a.taps;
            *bytes = B * a.Hin * a.Win * Cin * (a.in_nchw ? 4.0 : es) + opix * a.Cout * (a.out_nchw ? 4.0 : es) +
                     (double)a.Cout * Cin * a.taps * es + (a.res1 ? opix * a.Cout * es : 0.0);
            if (a.r_w) {  // the residual segment: its raw input once, its filter, its products
                const double Cres = a.r_C1 + a.r_C2;
                *flops += 2.0 * opix * a.Cout * Cres;
                *bytes += opix * Cres * es + (double)a.Cout * Cres * es;
            }
            break;
        }
        case OP_CAST: {
            const Tensor& ts = P->tensors[o.cast_src];
            snprintf(label, cap, "cast_f32_to_16_kernel");
            *bytes = B * ts.H * ts.W * ts.C * 6.0;
            break;
        }
        case OP_ATTN: {
            const Tensor& q = P->tensors[o.at_qkv];
            const double S = q.H * q.W, C = q.C / 3;
            if (P->x3 && attn_x3_supported(P->B, (int)S, (int)C, o.at_heads))
                snprintf(label, cap, "attn_x3_kernel");
            else if (o.at_heads > 1)
                snprintf(label, cap, attn_heads_mfma_supported(P->dtype, P->B, (int)S, (int)C, o.at_heads) ? "attn_mfma_kernel<%s,heads>" : S == 16 ? "attn_s16_kernel<%s,heads>" : "attn_generic_kernel<%s,heads>", tn);
            else
                snprintf(label, cap, !attn_mfma_supported(P->dtype, P->B, (int)S, (int)C) ? (S == 16 ? "attn_s16_kernel<%s>" : "attn_generic_kernel<%s>") : attn_full_takes((int)S, (int)C) ? "attn_full_kernel<%s>" : "attn_mfma_kernel<%s>", tn);
            *flops = 4.0 * B * S * S * C;
            *bytes = B * S * 4.0 * C * es;
            if (o.at_proj >= 0) {  // + the proj conv and the residual: context neither written nor read, residual in, output out
                snprintf(label, cap, "attn_full_kernel<%s,proj>", tn);
                *flops += 2.0 * B * S * C * C;
                *bytes = B * S * 5.0 * C * es + C * C * es;
            }
            break;
        }
    }
}


// ---- plan creation, phase by phase (dmme_unet_plan_create) -------------------------------------------------------------------------
static int check_cfg(const dmme_unet_cfg* cfg, int B, int H, int W, int dtype) {
    DMME_REQUIRE(B > 0 && H > 0 && W > 0, DMME_ERR_INVALID, "plan_create: bad shape B=%d H=%d W=%d", B, H, W);
    DMME_REQUIRE(dtype == DMME_F32 || dtype == DMME_BF16 || dtype == DMME_BF16X3 || dtype == DMME_F16 || dtype == DMME_F16R32, DMME_ERR_INVALID,
                 "plan_create: bad dtype %d", dtype);
    DMME_REQUIRE(cfg->num_depths >= 1 && cfg->num_depths <= 8 && cfg->num_blocks >= 1, DMME_ERR_INVALID,
                 "plan_create: bad depth/blocks");
    DMME_REQUIRE(cfg->num_attention_depths >= 0 && cfg->num_attention_depths <= 8, DMME_ERR_INVALID, "bad attention_depths");
    DMME_REQUIRE(cfg->pos_dim >= 4 && cfg->pos_dim % 2 == 0, DMME_ERR_INVALID, "pos_dim must be even and >= 4");
    DMME_REQUIRE(cfg->arch == DMME_ARCH_DDPM || cfg->arch == DMME_ARCH_IDDPM || cfg->arch == DMME_ARCH_CLASSIFIER || cfg->arch == DMME_ARCH_DDPM_COND,
                 DMME_ERR_INVALID, "plan_create: unknown arch %d", cfg->arch);
    if (cfg->arch == DMME_ARCH_DDPM_COND) {
        const bool x3 = dtype == DMME_BF16X3, mix = dtype == DMME_F16R32;
        DMME_REQUIRE(!x3 && !mix, DMME_ERR_UNSUPPORTED, "plan_create: the class-conditional UNet runs in fp32, bf16 or fp16 (not %s)", x3 ? "bf16x3" : "fp16r32");
        DMME_REQUIRE(cfg->num_classes >= 1, DMME_ERR_INVALID, "plan_create: class-conditional UNet with num_classes=%d", cfg->num_classes);
    }
    if (cfg->arch == DMME_ARCH_CLASSIFIER) {
        const bool x3 = dtype == DMME_BF16X3, mix = dtype == DMME_F16R32;
        DMME_REQUIRE(!x3 && !mix, DMME_ERR_UNSUPPORTED, "plan_create: the classifier runs in fp32, bf16 or fp16 (not %s)", x3 ? "bf16x3" : "fp16r32");
        DMME_REQUIRE(cfg->num_classes >= 1, DMME_ERR_INVALID, "plan_create: classifier num_classes=%d", cfg->num_classes);
        DMME_REQUIRE(cfg->channels_per_depth[cfg->num_depths - 1] <= 1024, DMME_ERR_UNSUPPORTED, "plan_create: classifier head wider than 1024 channels");
    }
    if (cfg->arch == DMME_ARCH_IDDPM) {
        DMME_REQUIRE(cfg->num_heads >= 1, DMME_ERR_INVALID, "plan_create: num_heads must be >= 1");
    }
    for (int d = 0; d < cfg->num_depths; ++d)
        DMME_REQUIRE(cfg->channels_per_depth[d] > 0 && cfg->channels_per_depth[d] % cfg->num_groups == 0,
                     DMME_ERR_INVALID, "channels_per_depth[%d]=%d not divisible by num_groups=%d", d,
                     cfg->channels_per_depth[d], cfg->num_groups);
    return DMME_OK;
}

// precision fp16r32: every conv of the fp32 level must have its kernel - there is no fall-back to a 16-bit path that would read fp32 as halves
static int check_mix_kernels(const dmme_plan* P) {
    if (!P->mix) return DMME_OK;
    for (const Op& o : P->ops) {
        if (o.kind != OP_CONV || !(o.mix || o.route_f32)) continue;
        ConvArgs a{};
        fill_conv(P, o, (const char*)4096, (const float*)4096, (float*)4096, (char*)4096, nullptr, 1, a);
        const bool ok = !o.mix || conv_route(P->dtype, a).family == (o.mix == 3 ? CONV_THIN : o.mix == 4 ? CONV1X1_SPLIT : CONV3X3_SPLIT);
        DMME_REQUIRE(ok, DMME_ERR_UNSUPPORTED, "plan_create: precision fp16r32 has no kernel for the %dx%d conv %d+%d -> %d channels on the %dx%d level (B = %d)",
                     o.taps == 9 ? 3 : 1, o.taps == 9 ? 3 : 1, a.C1, a.C2, a.Cout, a.Hout, a.Wout, P->B);
    }
    return DMME_OK;
}

static int count_launches(const dmme_plan* P, bool nograd = false) {
    int n = 0;
    for (const Op& o : P->ops) {
        if (o.fused_away || (nograd && o.folded_into >= 0)) continue;
        if (o.lvl >= 0)
            n += o.lvl_first;
        else if (o.kind == OP_GN)
            n += !(o.gn_direct || o.gn_in_consumer);
        else
            ++n;
    }
    return n;
}

#define DMME_TRY(expr)                 \
    do {                               \
        if (int rc_ = (expr)) return rc_; \
    } while (0)

// every table a device plan keeps on its device, and the pinned status word
static int upload_tables(dmme_plan* P) {
    DMME_CHECK_HIP(hipSetDevice(P->device));
    std::vector<PackItem> items, bitems, uitems;
    build_pack_items(P, items);
    build_pack_items_bwd(P, bitems);
    build_unpack_items(P, uitems);
    P->n_items = (int)items.size();
    P->n_items_bwd = (int)bitems.size();
    P->n_items_unpack = (int)uitems.size();
    DMME_TRY(P->items_dev.upload(items));
    DMME_TRY(P->items_bwd_dev.upload(bitems));
    DMME_TRY(P->items_unpack_dev.upload(uitems));
    DMME_TRY(P->tp_tiles_dev.upload(P->tp_tiles));
    DMME_TRY(P->col_jobs_dev.upload(P->col_jobs));
    DMME_TRY(P->bias_jobs_dev.upload(P->bias_jobs));
    if (!P->fold_jobs.empty()) DMME_TRY(P->fold_jobs_dev.upload(P->fold_jobs));
    std::vector<dmme_plan::WgGroup*> all_groups{&P->wg[0], &P->wg[1], &P->wg[2]};
    for (auto& B_ : P->gb)
        for (int k = 0; k < 3; ++k) all_groups.push_back(&B_.wg[k]);
    for (dmme_plan::WgGroup* G : all_groups) {
        if (G->jobs.empty()) continue;
        DMME_TRY(G->layers_dev.upload(G->layers));
        DMME_TRY(G->jobs_dev.upload(G->jobs));
    }
    // (every device plan: the backward reports a no-grad forward's workspace through this word too)
    DMME_TRY(P->err_host.alloc());
    for (LvlRun& R : P->lvl_runs) {
        DMME_TRY(R.ops_dev.upload(R.ops));
        if (R.raw_skipped > 0) DMME_TRY(R.ops_nograd_dev.upload(R.ops_nograd));
        DMME_TRY(R.sync_dev.zeroed(16 + R.ops.size() * 2 * (size_t)R.NG * LVL_NS));
    }
    return DMME_OK;
}

}  // namespace dmme

// ======================================================================== extern "C"
extern "C" {

DMME_API const char* dmme_last_error(void) { return g_err; }
DMME_API int dmme_version(void) { return 122; }  // 122: dmme_analytic_moment, dmme_analytic_vlb_rows; 121: DMME_CHAIN_PFODE, dmme_rademacher, dmme_pf_probe, dmme_chain_probe_pf, dmme_pf_dequantize, dmme_pf_scratch_floats, dmme_pf_dot, dmme_chain_dot_pf, dmme_pf_prior, dmme_pf_stage, dmme_chain_stage_pf, dmme_pf_chain_step, dmme_pf_ll_chain_step; 120: DMME_CHAIN_DPS, dmme_dps_capacity, dmme_dps_measure, dmme_dps_adjoint, dmme_chain_adjoint_dps, dmme_dps_step, dmme_chain_update_dps, dmme_dps_chain_step; 119: dmme_cm_target, dmme_cm_loss, dmme_ema_lerp; 118: DMME_CHAIN_DDNM, dmme_ddnm_measure, dmme_ddnm_step, dmme_chain_update_ddnm, dmme_ddnm_chain_step, dmme_ddnm_band_capacity; 117: dmme_distill_noise, dmme_distill_mid, dmme_distill_target; 116: DMME_CHAIN_ILVR, dmme_lowpass (+ _lds_capacity, _scratch_bytes), dmme_ilvr_step, dmme_chain_update_ilvr, dmme_ilvr_chain_step; 115: dmme_unet_pack_folded, dmme_unet_plan_num_launches_nograd / _num_folded, dmme_attention_fold, dmme_attention_block; 114: DMME_PRED_*, dmme_pred_to_eps, dmme_unet_plan_set_prediction, dmme_q_sample_pred, dmme_mse_loss_rows; 113: dmme_grid_tile; 112: DMME_CHAIN_REPAINT, dmme_repaint_step, dmme_chain_update_repaint, dmme_repaint_chain_step; 111: DMME_CHAIN_DPMPP / _DPMPP_CFG, dmme_dpmpp_step, dmme_chain_update_dpmpp, dmme_dpmpp_chain_step and their cfg forms, the loop state's history-valid word; 110: DMME_ARCH_DDPM_COND, dmme_unet_forward_cond / _backward_cond / _backward_input_cond, DMME_CHAIN_DDPM_CFG / _GDDIM_CFG, dmme_cfg_step, dmme_chain_update_cfg, dmme_cfg_chain_step, dmme_label_dropout; 109: dmme_iddpm_loss_rows, dmme_iddpm_prior_rows, dmme_tsampler_draw, dmme_tsampler_update; 108: DMME_CHAIN_GDDIM, dmme_gddim_step, dmme_chain_update_gddim, dmme_slerp; 107: DMME_ARCH_CLASSIFIER, dmme_unet_backward_input, guided chain; 106: dmme_unet_debug_read_grad; 105: dmme_attention_proj, dmme_unet_forward_nograd
DMME_API int dmme_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

DMME_API int dmme_unet_plan_create(const dmme_unet_cfg* cfg, int B, int H, int W, int dtype, int device, dmme_plan** out) {
    DMME_REQUIRE(cfg && out, DMME_ERR_INVALID, "plan_create: null argument");
    DMME_TRY(check_cfg(cfg, B, H, W, dtype));
    std::unique_ptr<dmme_plan> owned(new dmme_plan());  // (a failed create frees the plan and, through their types, its tables)
    dmme_plan* P = owned.get();
    P->cfg = *cfg;
    if (cfg->arch == DMME_ARCH_DDPM_COND) {  // the DDPM UNet plus one parameter: everything that asks for the architecture sees DDPM
        P->cond = 1;
        P->cfg.arch = DMME_ARCH_DDPM;
    }
    P->B = B;
    P->H = H;
    P->W = W;
    P->x3 = dtype == DMME_BF16X3;   // fp32 storage
    P->mix = dtype == DMME_F16R32;  // fp16 storage below the full-resolution level
    P->dtype = P->x3 ? DMME_F32 : P->mix ? DMME_F16 : dtype;
    P->device = device;
    DMME_TRY(build_plan(P));
    DMME_TRY(check_mix_kernels(P));
    assign_levels(P);
    const bool fused_gn = !getenv("DMME_NO_FUSED_GN");
    if (fused_gn) assign_stats(P);
    if (fused_gn && !getenv("DMME_NO_GN_DIRECT")) assign_direct(P);
    if (!getenv("DMME_NO_PREACT")) assign_preact(P);
    if (fused_gn) assign_gn_in(P);
    assign_rseg(P);
    assign_attn_proj(P);
    assign_lvl_nograd(P);
    assign_attn_fold(P);
    P->n_launches = count_launches(P);
    P->n_launches_nograd = count_launches(P, true);
    plan_backward(P);
    if (device >= 0) DMME_TRY(upload_tables(P));
    *out = owned.release();
    return DMME_OK;
}

DMME_API void dmme_unet_plan_destroy(dmme_plan* plan) { delete plan; }

DMME_API int dmme_unet_plan_num_params(const dmme_plan* plan) { return plan ? (int)plan->params.size() : 0; }

DMME_API int dmme_unet_plan_param_info(const dmme_plan* plan, int index, char* name, int name_cap, int* ndim,
                              int64_t shape[4], int64_t* ref_offset, int* is_buffer) {
    DMME_REQUIRE(plan && index >= 0 && index < (int)plan->params.size(), DMME_ERR_INVALID, "param_info: bad index %d", index);
    const Param& p = plan->params[index];
    if (name && name_cap > 0) {
        strncpy(name, p.name.c_str(), (size_t)name_cap - 1);
        name[name_cap - 1] = 0;
    }
    if (ndim) *ndim = p.ndim;
    if (shape)
        for (int i = 0; i < 4; ++i) shape[i] = p.shape[i];
    if (ref_offset) *ref_offset = p.ref_off;
    if (is_buffer) *is_buffer = p.is_buffer ? 1 : 0;
    return DMME_OK;
}

DMME_API int64_t dmme_unet_plan_ref_numel(const dmme_plan* plan) { return plan ? plan->ref_numel : 0; }
DMME_API int64_t dmme_unet_plan_packed_bytes(const dmme_plan* plan) { return plan ? plan->packed_bytes : 0; }
DMME_API int64_t dmme_unet_plan_workspace_bytes(const dmme_plan* plan) { return plan ? plan->ws_bytes : 0; }
DMME_API int64_t dmme_unet_plan_dropmask_numel(const dmme_plan* plan) { return plan ? plan->dropmask_numel : 0; }
DMME_API int dmme_unet_plan_out_channels(const dmme_plan* plan) { return plan ? plan->out_channels : 0; }
DMME_API int dmme_unet_plan_num_launches(const dmme_plan* plan) { return plan ? plan->n_launches : 0; }
DMME_API int dmme_unet_plan_num_launches_nograd(const dmme_plan* plan) { return plan ? plan->n_launches_nograd : 0; }
DMME_API int dmme_unet_plan_num_folded(const dmme_plan* plan) { return plan ? (int)plan->fold_jobs.size() : 0; }

DMME_API int dmme_unet_pack_params(const dmme_plan* plan, const float* ref_flat, void* packed, void* stream) {
    DMME_REQUIRE(plan && ref_flat && packed, DMME_ERR_INVALID, "pack_params: null argument");
    DMME_REQUIRE(plan->items_dev, DMME_ERR_INVALID, "pack_params: plan was created without a device");
    if (plan->fold_packed == packed) plan->fold_packed = nullptr;  // the folded slots describe the weights this call overwrites
    return launch_pack_table(plan->dtype, plan->items_dev.get(), plan->n_items, ref_flat, packed, (hipStream_t)stream);
}

// The folded attention matrices of `packed` (assign_attn_fold), from the 16-bit weights dmme_unet_pack_params left there: call it behind
// that, on the same stream, ahead of the no-grad forwards / chain steps of a weight version.  Until the next dmme_unet_pack_params of
// this buffer those walks then run their foldable blocks folded; with any other buffer, or without this call, they run unfolded.
DMME_API int dmme_unet_pack_folded(const dmme_plan* plan, void* packed, void* stream) {
    DMME_REQUIRE(plan && packed, DMME_ERR_INVALID, "pack_folded: null argument");
    DMME_REQUIRE(plan->items_dev, DMME_ERR_INVALID, "pack_folded: plan was created without a device");
    if (plan->fold_jobs.empty()) return DMME_OK;
    const int rc = launch_attn_fold_weights(plan->dtype, plan->fold_jobs_dev.get(), (int)plan->fold_jobs.size(), plan->fold_maxC, packed, (hipStream_t)stream);
    if (rc == DMME_OK) plan->fold_packed = packed;
    return rc;
}

// labels / status: the conditional form (dmme_unet_forward_cond); a conditional plan never runs without labels
static int unet_forward_impl(const dmme_plan* plan, const void* packed, const float* x, const int64_t* t, int t_len,
                      float* y, void* workspace, const float* drop_masks, void* stream, bool keep_ctx, const int64_t* labels = nullptr,
                      int* status = nullptr) {
    DMME_REQUIRE(plan && packed && x && t && y && workspace, DMME_ERR_INVALID, "unet_forward: null argument");
    DMME_REQUIRE((plan->cond != 0) == (labels != nullptr), DMME_ERR_INVALID,
                 plan->cond ? "unet_forward: a class-conditional plan (DMME_ARCH_DDPM_COND) takes labels: call dmme_unet_forward_cond / dmme_cfg_chain_step"
                            : "unet_forward_cond: the plan is not class-conditional (DMME_ARCH_DDPM_COND)");
    DMME_REQUIRE(t_len == 1 || t_len == plan->B, DMME_ERR_INVALID,
                 "unet_forward: timestep tensor of length %d does not broadcast against batch %d", t_len, plan->B);
    {
        const int rc = lvl_check(plan, "unet_forward", (hipStream_t)stream, true);
        if (rc != DMME_OK) return rc;
    }
    hipStream_t s = (hipStream_t)stream;
    const dmme_plan* P = plan;
    const char* pk = (const char*)packed;
    char* ws = (char*)workspace;
    const int nt = t_len;
    if (keep_ctx) {
        if (plan->nograd_ws == workspace) plan->nograd_ws = nullptr;
    } else {
        plan->nograd_ws = workspace;
    }
    for (int oi = 0; oi < (int)P->ops.size(); ++oi) {
        // behind the label op every image has its own time row, whatever t_len was
        const int rc = run_op(P, P->ops[oi], pk, x, t, P->cond && oi > P->label_op ? P->B : nt, y, ws, drop_masks, s, keep_ctx, labels, status);
        if (rc != DMME_OK) return rc;
    }
    if (P->head_src >= 0) {  // classifier head: GroupNorm + SiLU + spatial mean + Linear -> logits (B, K), one launch
        const Tensor& tt = P->tensors[P->head_src];
        return launch_cls_head_fwd(P->dtype, ws + tt.off, P->B, tt.H * tt.W, tt.C, P->cfg.num_groups, (const float*)(pk + P->params[P->p_hgw].packed_off),
                                   (const float*)(pk + P->params[P->p_hgb].packed_off), (const float*)(pk + P->params[P->p_hw].packed_off),
                                   (const float*)(pk + P->params[P->p_hb].packed_off), P->out_channels, y, s);
    }
    return DMME_OK;
}
DMME_API int dmme_unet_forward(const dmme_plan* plan, const void* packed, const float* x, const int64_t* t, int t_len,
                      float* y, void* workspace, const float* drop_masks, void* stream) {
    return unet_forward_impl(plan, packed, x, t, t_len, y, workspace, drop_masks, stream, true);
}
// the same forward where no backward pass will follow (sampling, evaluation under no_grad): tensors only a backward pass reads - the
// context of an attention block whose proj conv runs inside the attention launch - are not written
DMME_API int dmme_unet_forward_nograd(const dmme_plan* plan, const void* packed, const float* x, const int64_t* t, int t_len,
                      float* y, void* workspace, const float* drop_masks, void* stream) {
    return unet_forward_impl(plan, packed, x, t, t_len, y, workspace, drop_masks, stream, false);
}

DMME_API int dmme_unet_forward_cond(const dmme_plan* plan, const void* packed, const float* x, const int64_t* t, int t_len, const int64_t* labels,
                                    float* y, void* workspace, const float* drop_masks, int keep_ctx, int* status, void* stream) {
    DMME_REQUIRE(labels, DMME_ERR_INVALID, "unet_forward_cond: null argument (labels)");
    return unet_forward_impl(plan, packed, x, t, t_len, y, workspace, drop_masks, stream, keep_ctx != 0, labels, status);
}

DMME_API int dmme_unet_plan_num_ops(const dmme_plan* plan) { return plan ? (int)plan->ops.size() : 0; }

DMME_API int dmme_unet_plan_op_info(const dmme_plan* plan, int index, char* label, int label_cap, double* flops,
                                    double* bytes) {
    DMME_REQUIRE(plan && index >= 0 && index < (int)plan->ops.size() && label && label_cap > 0 && flops && bytes,
                 DMME_ERR_INVALID, "op_info: bad argument");
    op_account(plan, plan->ops[index], label, label_cap, flops, bytes);
    return DMME_OK;
}

DMME_API int dmme_unet_forward_profiled(const dmme_plan* plan, const void* packed, const float* x, const int64_t* t,
                                        int t_len, float* y, void* workspace, const float* drop_masks, void* stream,
                                        float* op_ms) {
    DMME_REQUIRE(plan && packed && x && t && y && workspace && op_ms, DMME_ERR_INVALID, "forward_profiled: null argument");
    DMME_REQUIRE(t_len == 1 || t_len == plan->B, DMME_ERR_INVALID, "forward_profiled: bad t_len %d", t_len);
    DMME_REQUIRE(!plan->cond, DMME_ERR_INVALID, "forward_profiled: a class-conditional plan takes labels (dmme_unet_forward_cond); this entry point has none");
    if (int rc0 = lvl_check(plan, "forward_profiled", (hipStream_t)stream, true)) return rc0;
    hipStream_t s = (hipStream_t)stream;
    const size_t n = plan->ops.size();
    plan->nograd_ws = workspace;
    std::vector<hipEvent_t> ev(n + 1);
    for (auto& e : ev) DMME_CHECK_HIP(hipEventCreate(&e));
    int rc = DMME_OK;
    DMME_CHECK_HIP(hipEventRecord(ev[0], s));
    for (size_t i = 0; i < n && rc == DMME_OK; ++i) {
        rc = run_op(plan, plan->ops[i], (const char*)packed, x, t, t_len, y, (char*)workspace, drop_masks, s, false);  // (the sampling step's forward)
        if (rc == DMME_OK && hipEventRecord(ev[i + 1], s) != hipSuccess) rc = DMME_ERR_HIP;
    }
    if (rc == DMME_OK && hipEventSynchronize(ev[n]) != hipSuccess) rc = DMME_ERR_HIP;
    for (size_t i = 0; i < n && rc == DMME_OK; ++i)
        if (hipEventElapsedTime(&op_ms[i], ev[i], ev[i + 1]) != hipSuccess) rc = DMME_ERR_HIP;
    for (auto& e : ev) (void)hipEventDestroy(e);
    if (rc == DMME_ERR_HIP) set_error("forward_profiled: HIP event error");
    return rc;
}

// ---------------------------------------------------------------- training: backward + optimiser
DMME_API int dmme_grad_norm(const float* grad, int64_t numel, float* norm_out, float* scratch, void* stream) {
    DMME_REQUIRE(grad && norm_out && scratch && numel > 0, DMME_ERR_INVALID, "grad_norm: bad argument");
    return launch_grad_norm(grad, numel, norm_out, scratch, (hipStream_t)stream);
}

DMME_API int dmme_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* ema, int64_t numel, float lr,
                            float beta1, float beta2, float eps, int step, const float* grad_norm, float max_norm, float ema_decay,
                            float grad_scale, void* stream) {
    DMME_REQUIRE(param && grad && exp_avg && exp_avg_sq && numel > 0 && step >= 1 && grad_scale > 0.f, DMME_ERR_INVALID, "adam_step: bad argument");
    return launch_adam(param, grad, exp_avg, exp_avg_sq, ema, numel, lr, beta1, beta2, eps, step, grad_norm, max_norm, ema_decay, grad_scale,
                       (hipStream_t)stream);
}

DMME_API int dmme_amp_init(float* amp_state, float init_scale, void* stream) {
    DMME_REQUIRE(amp_state && init_scale > 0.f, DMME_ERR_INVALID, "amp_init: bad argument");
    return launch_amp_init(amp_state, init_scale, (hipStream_t)stream);
}
DMME_API int dmme_amp_scale(float* grad, int64_t numel, const float* amp_state, void* stream) {
    DMME_REQUIRE(grad && amp_state && numel >= 0, DMME_ERR_INVALID, "amp_scale: bad argument");
    return launch_amp_scale(grad, numel, amp_state, (hipStream_t)stream);
}
DMME_API int dmme_adam_step_amp(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* ema, int64_t numel, float lr, float beta1,
                                float beta2, float eps, const float* grad_norm, float max_grad_norm, float ema_decay, float grad_scale,
                                float* amp_state, float growth_factor, float backoff_factor, int growth_interval, void* stream) {
    DMME_REQUIRE(param && grad && exp_avg && exp_avg_sq && grad_norm && amp_state, DMME_ERR_INVALID, "adam_step_amp: null argument");
    DMME_REQUIRE(numel > 0 && grad_scale > 0.f, DMME_ERR_INVALID, "adam_step_amp: bad argument");  // (numel 0 would be a zero-block launch)
    DMME_REQUIRE(growth_factor >= 1.f && backoff_factor > 0.f && backoff_factor <= 1.f && growth_interval >= 1, DMME_ERR_INVALID, "adam_step_amp: bad scaler constants");
    return launch_adam_amp(param, grad, exp_avg, exp_avg_sq, ema, numel, lr, beta1, beta2, eps, grad_norm, max_grad_norm, ema_decay, grad_scale, amp_state,
                           growth_factor, backoff_factor, growth_interval, (hipStream_t)stream);
}

DMME_API int dmme_grad_pack_bf16(const float* grad, int64_t numel, void* dst_bf16, int64_t numel_padded, void* stream) {
    DMME_REQUIRE(grad && dst_bf16 && numel > 0 && numel_padded >= numel, DMME_ERR_INVALID, "grad_pack_bf16: bad argument");
    return launch_grad_pack_bf16(grad, numel, dst_bf16, numel_padded, (hipStream_t)stream);
}
DMME_API int dmme_shard_reduce_bf16(const void* recv_bf16, int world, int64_t per_rank, float scale, void* out_bf16, void* stream) {
    DMME_REQUIRE(recv_bf16 && out_bf16 && world >= 1 && per_rank > 0, DMME_ERR_INVALID, "shard_reduce_bf16: bad argument");
    return launch_shard_reduce_bf16(recv_bf16, world, per_rank, scale, out_bf16, (hipStream_t)stream);
}
DMME_API int dmme_grad_unpack_bf16(const void* src_bf16, int64_t numel, float* grad, void* stream) {
    DMME_REQUIRE(src_bf16 && grad && numel > 0, DMME_ERR_INVALID, "grad_unpack_bf16: bad argument");
    return launch_grad_unpack_bf16(src_bf16, numel, grad, (hipStream_t)stream);
}

DMME_API int dmme_unet_debug_read(const dmme_plan* plan, const void* workspace, const char* name, float* dst,
                         int64_t numel_cap, int64_t* numel_out, void* stream) {
    DMME_REQUIRE(plan && workspace && name && dst, DMME_ERR_INVALID, "debug_read: null argument");
    hipStream_t s = (hipStream_t)stream;
    if (strcmp(name, "condition") == 0) {
        const int64_t n = (int64_t)plan->B * plan->cfg.emb_dim;  // rows beyond t_len are unspecified
        DMME_REQUIRE(n <= numel_cap, DMME_ERR_INVALID, "debug_read: destination too small");
        DMME_CHECK_HIP(hipMemcpyAsync(dst, (const char*)workspace + plan->ws_temb, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
        if (numel_out) *numel_out = n;
        return DMME_OK;
    }
    auto it = plan->named.find(name);
    DMME_REQUIRE(it != plan->named.end(), DMME_ERR_INVALID, "debug_read: unknown module '%s'", name);
    const Tensor& t = plan->tensors[it->second];
    const int64_t n = (int64_t)plan->B * t.C * t.H * t.W;
    DMME_REQUIRE(n <= numel_cap, DMME_ERR_INVALID, "debug_read: destination too small (%lld > %lld)", (long long)n,
                 (long long)numel_cap);
    if (numel_out) *numel_out = n;
    return launch_nhwc_to_nchw(t.f32 ? DMME_F32 : plan->dtype, (const char*)workspace + t.off, plan->B, t.C, t.H * t.W, dst, s);
}

// gradient buffers of the reverse walk (plan_bwd.hip): every forward tensor has its own (gt_off); the aliases the plan sets up share a
// buffer only between tensors whose gradients are equal (a block's 1x1 residual output and the block output), so after
// dmme_unet_backward the buffer of every named tensor holds its full gradient.  The time embedding's is the exception: the MLP backward
// turns d(temb) into d(pre-activation) in place.
DMME_API int dmme_unet_debug_read_grad(const dmme_plan* plan, const void* bwd_workspace, const char* name, float* dst,
                                       int64_t numel_cap, int64_t* numel_out, void* stream) {
    DMME_REQUIRE(plan && bwd_workspace && name && dst, DMME_ERR_INVALID, "debug_read_grad: null argument");
    DMME_REQUIRE(strcmp(name, "condition") != 0, DMME_ERR_INVALID,
                 "debug_read_grad: the gradient of 'condition' is not kept (the time-MLP backward overwrites it in place with the gradient "
                 "of the pre-activation); compare the condition.* parameter gradients instead");
    auto it = plan->named.find(name);
    DMME_REQUIRE(it != plan->named.end(), DMME_ERR_INVALID, "debug_read_grad: unknown module '%s'", name);
    const Tensor& t = plan->tensors[it->second];
    const int64_t n = (int64_t)plan->B * t.C * t.H * t.W;
    DMME_REQUIRE(n <= numel_cap, DMME_ERR_INVALID, "debug_read_grad: destination too small (%lld > %lld)", (long long)n,
                 (long long)numel_cap);
    if (numel_out) *numel_out = n;
    return launch_nhwc_to_nchw(plan->dtype, (const char*)bwd_workspace + plan->gt_off[it->second], plan->B, t.C, t.H * t.W, dst,
                               (hipStream_t)stream);
}

// {mean, rstd} rows of a GroupNorm as the forward left them for the backward (Op::gn_mr), by the norm's state_dict prefix
DMME_API int dmme_unet_debug_read_norm_stats(const dmme_plan* plan, const void* workspace, const char* name, float* dst,
                                             int64_t numel_cap, int64_t* numel_out, void* stream) {
    DMME_REQUIRE(plan && workspace && name && dst, DMME_ERR_INVALID, "debug_read_norm_stats: null argument");
    const std::string key = std::string(name) + ".weight";
    for (const Op& o : plan->ops) {
        if (o.kind != OP_GN || o.gn_gamma < 0 || plan->params[o.gn_gamma].name != key) continue;
        const int64_t n = (int64_t)plan->B * plan->cfg.num_groups * 2;
        DMME_REQUIRE(n <= numel_cap, DMME_ERR_INVALID, "debug_read_norm_stats: destination too small (%lld > %lld)", (long long)n,
                     (long long)numel_cap);
        DMME_CHECK_HIP(hipMemcpyAsync(dst, (const char*)workspace + o.gn_mr, (size_t)n * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
        if (numel_out) *numel_out = n;
        return DMME_OK;
    }
    set_error("debug_read_norm_stats: no GroupNorm named '%s'", name);
    return DMME_ERR_INVALID;
}

DMME_API int dmme_dropout_masks(const dmme_plan* plan, uint64_t seed, uint64_t offset, float* masks, void* stream) {
    DMME_REQUIRE(plan && masks, DMME_ERR_INVALID, "dropout_masks: null argument");
    return launch_dropmask(masks, plan->dropmask_numel, plan->cfg.dropout, seed, offset, (hipStream_t)stream);
}

DMME_API int dmme_randn(float* out, int64_t numel, uint64_t seed, uint64_t offset, void* stream) {
    DMME_REQUIRE(out && numel >= 0, DMME_ERR_INVALID, "randn: bad argument");
    return launch_randn(out, numel, seed, offset, (hipStream_t)stream);
}

DMME_API int dmme_q_sample(const float* x0, const float* z, const float* sqrt_abar, const float* sqrt_1m_abar,
                           const int64_t* t, int B, int64_t chw, float* x_t, float* target, void* stream) {
    DMME_REQUIRE(x0 && z && sqrt_abar && sqrt_1m_abar && t && x_t && B > 0 && chw > 0, DMME_ERR_INVALID, "q_sample: bad argument");
    return launch_q_sample(x0, z, sqrt_abar, sqrt_1m_abar, t, B, chw, x_t, target, (hipStream_t)stream);
}

// ---- the reverse updates (kernels_sampler.hip): every entry point fills in the operands of its kind and calls one of two launchers
static SamplerOperands sampler_operands(float* x, const float* out, const float* zin, int64_t B, int64_t chw, const float* grad = nullptr,
                                        float* hist = nullptr, int planes = 1, const float* known = nullptr, const float* mask = nullptr) {
    return SamplerOperands{x, out, grad, zin, hist, known, mask, chw, B * chw, (B * chw + 3) / 4, planes};
}

DMME_API int dmme_ddpm_step(float* x, const float* eps, const float* z, float inv_sqrt_alpha, float eps_coef, float sigma,
                   int add_noise, int64_t numel, void* stream) {
    DMME_REQUIRE(x && eps && (z || !add_noise), DMME_ERR_INVALID, "ddpm_step: null argument");
    const float row[4] = {inv_sqrt_alpha, eps_coef, sigma, 0.f};
    return launch_sampler_eager("ddpm_step", DMME_CHAIN_DDPM, sampler_operands(x, eps, z, 1, numel), row, add_noise, (hipStream_t)stream);
}

DMME_API int dmme_ddim_step(float* x, const float* eps, float sqrt_one_minus_abar, float sqrt_abar_prev, int64_t numel,
                   void* stream) {
    DMME_REQUIRE(x && eps, DMME_ERR_INVALID, "ddim_step: null argument");
    const float row[4] = {sqrt_one_minus_abar, sqrt_abar_prev, 0.f, 0.f};
    return launch_sampler_eager("ddim_step", DMME_CHAIN_DDIM, sampler_operands(x, eps, nullptr, 1, numel), row, 0, (hipStream_t)stream);
}

DMME_API int dmme_gddim_step(float* x, const float* eps, const float* z, float k0, float k1, float k2, int64_t numel, void* stream) {
    DMME_REQUIRE(x && eps && (z || k2 == 0.0f) && numel >= 0, DMME_ERR_INVALID, "gddim_step: null argument (z is needed where k2 != 0)");
    const float row[4] = {k0, k1, k2, 0.f};
    return launch_sampler_eager("gddim_step", DMME_CHAIN_GDDIM, sampler_operands(x, eps, z, 1, numel), row, 0, (hipStream_t)stream);
}

DMME_API int dmme_iddpm_step(float* x, const float* model_out, const float* z, float inv_sqrt_alpha, float eps_coef, float log_beta,
                             float log_beta_tilde, int add_noise, int B, int64_t chw, void* stream) {
    DMME_REQUIRE(x && model_out && (z || !add_noise) && B > 0 && chw > 0, DMME_ERR_INVALID, "iddpm_step: bad argument");
    const float row[4] = {inv_sqrt_alpha, eps_coef, log_beta, log_beta_tilde};
    return launch_sampler_eager("iddpm_step", DMME_CHAIN_IDDPM, sampler_operands(x, model_out, z, B, chw), row, add_noise, (hipStream_t)stream);
}

DMME_API int dmme_chain_set(void* state, int64_t i, const int64_t* t_table, uint64_t philox_seed, uint64_t philox_offset, void* stream) {
    DMME_REQUIRE(state && t_table && i >= 0, DMME_ERR_INVALID, "chain_set: bad argument");
    return launch_chain_set(state, i, t_table, philox_seed, philox_offset, (hipStream_t)stream);
}

DMME_API int dmme_chain_update(int kind, float* x, const float* model_out, const float* step_coef, const int64_t* t_table, void* state,
                               int B, int64_t chw, void* stream) {
    DMME_REQUIRE(x && model_out && step_coef && t_table && state && B > 0 && chw > 0, DMME_ERR_INVALID, "chain_update: bad argument");
    DMME_REQUIRE(kind >= DMME_CHAIN_DDPM && kind <= DMME_CHAIN_GDDIM, DMME_ERR_INVALID, "chain_update: unknown sampler kind %d", kind);
    return launch_sampler_chain("chain_update", kind, sampler_operands(x, model_out, nullptr, B, chw), step_coef, t_table, state, (hipStream_t)stream);
}

DMME_API int dmme_chain_update_gddim(float* x, const float* model_out, const float* noise, const float* step_coef, const int64_t* t_table,
                                     void* state, int B, int64_t chw, void* stream) {
    DMME_REQUIRE(x && model_out && step_coef && t_table && state && B > 0 && chw > 0, DMME_ERR_INVALID, "chain_update_gddim: bad argument");
    return launch_sampler_chain("chain_update_gddim", DMME_CHAIN_GDDIM, sampler_operands(x, model_out, noise, B, chw), step_coef, t_table, state,
                                (hipStream_t)stream);
}

DMME_API int dmme_chain_update_guided(int kind, float* x, const float* model_out, const float* grad, const float* noise, const float* step_coef,
                                      const int64_t* t_table, void* state, int B, int64_t chw, void* stream) {
    DMME_REQUIRE(x && model_out && grad && step_coef && t_table && state && B > 0 && chw > 0, DMME_ERR_INVALID, "chain_update_guided: bad argument");
    DMME_REQUIRE(kind_grad(kind), DMME_ERR_INVALID, "chain_update_guided: kind %d is not a guided kind", kind);
    return launch_sampler_chain("chain_update_guided", kind, sampler_operands(x, model_out, noise, B, chw, grad), step_coef, t_table, state,
                                (hipStream_t)stream);
}

static bool kind_plain_cfg(int kind) { return kind == DMME_CHAIN_DDPM_CFG || kind == DMME_CHAIN_GDDIM_CFG; }
DMME_API int dmme_cfg_step(int kind, float* x, const float* model_out, const float* z, float c0, float c1, float c2, float s, int add_noise, int B,
                           int64_t chw, void* stream) {
    DMME_REQUIRE(kind_plain_cfg(kind), DMME_ERR_INVALID, "cfg_step: kind %d is not a classifier-free kind (6, 7)", kind);
    const float row[4] = {c0, c1, c2, s};
    return launch_sampler_eager("cfg_step", kind, sampler_operands(x, model_out, z, B, chw), row, add_noise, (hipStream_t)stream);
}

DMME_API int dmme_chain_update_cfg(int kind, float* x, const float* model_out, const float* noise, const float* step_coef, const int64_t* t_table,
                                   void* state, int B, int64_t chw, void* stream) {
    DMME_REQUIRE(kind_plain_cfg(kind), DMME_ERR_INVALID, "chain_update_cfg: kind %d is not a classifier-free kind (6, 7)", kind);
    return launch_sampler_chain("chain_update_cfg", kind, sampler_operands(x, model_out, noise, B, chw), step_coef, t_table, state, (hipStream_t)stream);
}

// DPM-Solver++(2M): kinds DMME_CHAIN_DPMPP / DMME_CHAIN_DPMPP_CFG, tables of 8 floats per index, a history buffer
DMME_API int dmme_dpmpp_step(float* x, const float* model_out, float* history, const float* row, int history_valid, int B, int64_t chw, int out_planes,
                             void* stream) {
    return launch_sampler_eager("dpmpp_step", DMME_CHAIN_DPMPP, sampler_operands(x, model_out, nullptr, B, chw, nullptr, history, out_planes), row,
                                history_valid, (hipStream_t)stream);
}

DMME_API int dmme_chain_update_dpmpp(float* x, const float* model_out, float* history, const float* step_coef, const int64_t* t_table, void* state, int B,
                                     int64_t chw, int out_planes, void* stream) {
    return launch_sampler_chain("chain_update_dpmpp", DMME_CHAIN_DPMPP, sampler_operands(x, model_out, nullptr, B, chw, nullptr, history, out_planes),
                                step_coef, t_table, state, (hipStream_t)stream);
}

DMME_API int dmme_cfg_dpmpp_step(float* x_2B, const float* model_out, float* history, const float* row, int history_valid, int B, int64_t chw, void* stream) {
    return launch_sampler_eager("cfg_dpmpp_step", DMME_CHAIN_DPMPP_CFG, sampler_operands(x_2B, model_out, nullptr, B, chw, nullptr, history), row, history_valid,
                                (hipStream_t)stream);
}

DMME_API int dmme_chain_update_cfg_dpmpp(float* x_2B, const float* model_out, float* history, const float* step_coef, const int64_t* t_table, void* state,
                                         int B, int64_t chw, void* stream) {
    return launch_sampler_chain("chain_update_cfg_dpmpp", DMME_CHAIN_DPMPP_CFG, sampler_operands(x_2B, model_out, nullptr, B, chw, nullptr, history), step_coef,
                                t_table, state, (hipStream_t)stream);
}

// RePaint / SDEdit: kind DMME_CHAIN_REPAINT, tables of 8 floats per index, the known image and its mask, three normal streams per step
DMME_API int dmme_repaint_step(float* x, const float* model_out, const float* known, const float* mask, const float* z3, const float* row, int B,
                               int64_t chw, int out_planes, void* stream) {
    return launch_sampler_eager("repaint_step", DMME_CHAIN_REPAINT, sampler_operands(x, model_out, z3, B, chw, nullptr, nullptr, out_planes, known, mask), row, 0,
                                (hipStream_t)stream);
}

DMME_API int dmme_chain_update_repaint(float* x, const float* model_out, const float* known, const float* mask, const float* noise,
                                       const float* step_coef, const int64_t* t_table, void* state, int B, int64_t chw, int out_planes, void* stream) {
    return launch_sampler_chain("chain_update_repaint", DMME_CHAIN_REPAINT, sampler_operands(x, model_out, noise, B, chw, nullptr, nullptr, out_planes, known, mask),
                                step_coef, t_table, state, (hipStream_t)stream);
}

// The front half of a capturable step, shared by every kind: the checks of the plan (`cfg`: a classifier-free kind; want_planes: the
// output planes per image the kind takes, 0 = one or two), the forward, the x0 / v adapter, x0 thresholding (row, scol: where a
// classifier-free kind's table holds its scale).  planes: the network's output planes per image.  keep: the forward is the form a
// backward can follow (dmme_dps_chain_step); every other step runs the no-grad form.
static int chain_step_front(const char* what, const dmme_plan* plan, const void* packed, float* x, const int64_t* labels, int* status, float* model_out,
                            void* workspace, int kind, bool cfg, int want_planes, const float* step_coef, int row, int scol, void* state, void* stream,
                            int& planes, bool keep = false) {
    if (cfg)
        DMME_REQUIRE(plan->cond && plan->B % 2 == 0, DMME_ERR_INVALID,
                     "%s: needs a class-conditional plan (DMME_ARCH_DDPM_COND) of even batch: conditional half, unconditional half (B = %d)", what, plan->B);
    else
        DMME_REQUIRE(!plan->cond, DMME_ERR_INVALID, "%s: a class-conditional plan takes labels: call dmme_cfg_chain_step / dmme_cfg_dpmpp_chain_step", what);
    DMME_REQUIRE(plan->cfg.arch != DMME_ARCH_CLASSIFIER, DMME_ERR_INVALID, "%s: architecture %d predicts no noise", what, plan->cfg.arch);
    planes = plan->out_channels / plan->cfg.in_channels;
    DMME_REQUIRE(plan->out_channels == planes * plan->cfg.in_channels && (want_planes ? planes == want_planes : planes == 1 || planes == 2),
                 DMME_ERR_INVALID, "%s: sampler kind %d does not fit a network with %d output channels for %d input channels", what, kind, plan->out_channels,
                 plan->cfg.in_channels);
    if (!cfg)
        if (int rc = lvl_check(plan, what, (hipStream_t)stream, true)) return rc;
    const int64_t* t_dev = (const int64_t*)state + 1;
    if (int rc = unet_forward_impl(plan, packed, x, t_dev, 1, model_out, workspace, nullptr, stream, keep, labels, status)) return rc;
    // an x0 / v network: its output becomes an eps prediction here, over the plan's whole batch (a classifier-free plan's 2B images: the
    // affine map commutes with the guidance mix), and everything behind this line is the eps code
    if (plan->pred != DMME_PRED_EPS)
        if (int rc = launch_pred_to_eps(plan->pred, model_out, x, plan->pred_ab, plan->pred_T, t_dev, 1, plan->B,
                                        (int64_t)plan->cfg.in_channels * plan->H * plan->W, (hipStream_t)stream))
            return rc;
    // x0 thresholding: the eps plane the update will read (a classifier-free kind: the update's own mix of the two halves, its scale read
    // from the step's table row on the device) rewritten so that the x0 it implies is clipped; off launches nothing
    if (plan->thr_mode != DMME_THRESHOLD_NONE)
        if (int rc = launch_x0_threshold(plan->thr_mode, model_out, x, plan->thr_table, plan->thr_T, t_dev, 1, cfg ? plan->B / 2 : plan->B,
                                         (int64_t)plan->cfg.in_channels * plan->H * plan->W, planes, cfg ? 2 : 1, 1.0f, cfg ? step_coef : nullptr, row, scol,
                                         (const int64_t*)state, plan->thr_k, plan->thr_frac, plan->thr_scratch, (hipStream_t)stream))
            return rc;
    return DMME_OK;
}

// One capturable step of any kind: the checks of plan against kind, the network's no-grad forward at the device-resident t (the loop
// state's second word), `between` (the guided kinds' classifier pass, which fills the gradient operand), the update.  A classifier-free kind
// runs a class-conditional plan of batch 2B with labels (conditional half, unconditional half) and updates at B = plan batch / 2.
// The forward looks at the level engine's status word itself, under the name unet_forward; the unconditional entry points have always
// looked first under their own name, and still do.
static int chain_step_common(const char* what, const dmme_plan* plan, const void* packed, float* x, const int64_t* labels, int* status, float* model_out,
                             void* workspace, int kind, const float* grad, float* hist, const float* step_coef, const int64_t* t_table, void* state,
                             void* stream, const std::function<int()>& between = nullptr, const float* known = nullptr, const float* mask = nullptr) {
    const bool cfg = kind_cfg(kind);
    DMME_REQUIRE(plan && packed && x && model_out && workspace && step_coef && t_table && state && (labels || !cfg) && (hist || !kind_hist(kind)) &&
                     ((known && mask) || !kind_paint(kind)),
                 DMME_ERR_INVALID, "%s: null argument", what);
    int planes = 0;
    if (int rc = chain_step_front(what, plan, packed, x, labels, status, model_out, workspace, kind, cfg, kind_planes(kind), step_coef, kind_row(kind),
                                  kind_scol(kind), state, stream, planes))
        return rc;
    if (between)
        if (int rc = between()) return rc;
    return launch_sampler_chain(what, kind, sampler_operands(x, model_out, nullptr, cfg ? plan->B / 2 : plan->B, (int64_t)plan->cfg.in_channels * plan->H * plan->W,
                                                             grad, hist, planes, known, mask),
                                step_coef, t_table, state, (hipStream_t)stream);
}

DMME_API int dmme_chain_step(const dmme_plan* plan, const void* packed, float* x, float* model_out, void* workspace, int kind,
                             const float* step_coef, const int64_t* t_table, void* state, void* stream) {
    DMME_REQUIRE(kind_known(kind) && !kind_cfg(kind) && !kind_grad(kind) && !kind_hist(kind) && !kind_paint(kind), DMME_ERR_INVALID,
                 "chain_step: sampler kind %d (guided kinds: dmme_guided_chain_step, and so on)", kind);
    return chain_step_common("chain_step", plan, packed, x, nullptr, nullptr, model_out, workspace, kind, nullptr, nullptr, step_coef, t_table, state, stream);
}

// Ho & Salimans 2021 as one launch sequence: both halves in one forward at batch 2B, then the mixing update
DMME_API int dmme_cfg_chain_step(const dmme_plan* plan_2B, const void* packed, float* x_2B, const int64_t* labels_2B, float* model_out, void* workspace,
                                 int* status, int kind, const float* step_coef, const int64_t* t_table, void* state, void* stream) {
    DMME_REQUIRE(kind_plain_cfg(kind), DMME_ERR_INVALID, "cfg_chain_step: kind %d is not a classifier-free kind (6, 7)", kind);
    return chain_step_common("cfg_chain_step", plan_2B, packed, x_2B, labels_2B, status, model_out, workspace, kind, nullptr, nullptr, step_coef, t_table, state,
                             stream);
}

DMME_API int dmme_dpmpp_chain_step(const dmme_plan* plan, const void* packed, float* x, float* model_out, void* workspace, float* history,
                                   const float* step_coef, const int64_t* t_table, void* state, void* stream) {
    return chain_step_common("dpmpp_chain_step", plan, packed, x, nullptr, nullptr, model_out, workspace, DMME_CHAIN_DPMPP, nullptr, history, step_coef, t_table,
                             state, stream);
}

DMME_API int dmme_cfg_dpmpp_chain_step(const dmme_plan* plan_2B, const void* packed, float* x_2B, const int64_t* labels_2B, float* model_out, void* workspace,
                                       int* status, float* history, const float* step_coef, const int64_t* t_table, void* state, void* stream) {
    return chain_step_common("cfg_dpmpp_chain_step", plan_2B, packed, x_2B, labels_2B, status, model_out, workspace, DMME_CHAIN_DPMPP_CFG, nullptr, history,
                             step_coef, t_table, state, stream);
}

DMME_API int dmme_repaint_chain_step(const dmme_plan* plan, const void* packed, float* x, float* model_out, void* workspace, const float* known,
                                     const float* mask, const float* step_coef, const int64_t* t_table, void* state, void* stream) {
    return chain_step_common("repaint_chain_step", plan, packed, x, nullptr, nullptr, model_out, workspace, DMME_CHAIN_REPAINT, nullptr, nullptr, step_coef, t_table,
                             state, stream, nullptr, known, mask);
}

// ILVR: kind DMME_CHAIN_ILVR, whose update works on whole planes (csrc/ilvr.hip) behind the front half every chain step has
DMME_API int dmme_ilvr_chain_step(const dmme_plan* plan, const void* packed, float* x, float* model_out, void* workspace, const float* ref, const float* Ph,
                                  const float* Pw, float* scratch, const float* step_coef, const int64_t* t_table, void* state, void* stream) {
    DMME_REQUIRE(plan && packed && x && model_out && workspace && ref && Ph && Pw && step_coef && t_table && state, DMME_ERR_INVALID,
                 "ilvr_chain_step: null argument");
    int planes = 0;
    if (int rc = chain_step_front("ilvr_chain_step", plan, packed, x, nullptr, nullptr, model_out, workspace, DMME_CHAIN_ILVR, false, 0, nullptr, 8, 0, state,
                                  stream, planes))
        return rc;
    return launch_ilvr("ilvr_chain_step", x, model_out, ref, nullptr, nullptr, Ph, Pw, scratch, step_coef, t_table, state, plan->B, plan->cfg.in_channels, plan->H,
                       plan->W, planes, 0, (hipStream_t)stream);
}

// DDNM: kind DMME_CHAIN_DDNM, whose update reduces over measurement cells (csrc/ddnm.hip) behind the front half every chain step has
DMME_API int dmme_ddnm_chain_step(const dmme_plan* plan, const void* packed, float* x, float* model_out, void* workspace, const float* y, const float* mask,
                                  int s, int gray, const float* step_coef, const int64_t* t_table, void* state, void* stream) {
    DMME_REQUIRE(plan && packed && x && model_out && workspace && y && mask && step_coef && t_table && state, DMME_ERR_INVALID,
                 "ddnm_chain_step: null argument");
    int planes = 0;
    if (int rc = chain_step_front("ddnm_chain_step", plan, packed, x, nullptr, nullptr, model_out, workspace, DMME_CHAIN_DDNM, false, 0, nullptr, 8, 0, state,
                                  stream, planes))
        return rc;
    return launch_ddnm("ddnm_chain_step", x, model_out, y, mask, nullptr, nullptr, step_coef, t_table, state, plan->B, plan->cfg.in_channels, plan->H, plan->W, s,
                       gray, planes, (hipStream_t)stream);
}

// what the steps that differentiate the denoiser (DPS, the likelihood's stage) ask of their plan
static int require_differentiable_plan(const char* what, const dmme_plan* plan) {
    DMME_REQUIRE(!plan->cond && (plan->cfg.arch == DMME_ARCH_DDPM || plan->cfg.arch == DMME_ARCH_IDDPM), DMME_ERR_INVALID,
                 "%s: needs an unconditional DMME_ARCH_DDPM or DMME_ARCH_IDDPM plan (got architecture %d%s)", what, plan->cfg.arch,
                 plan->cond ? ", class-conditional" : "");
    DMME_REQUIRE(plan->pred == DMME_PRED_EPS, DMME_ERR_UNSUPPORTED,
                 "%s: the plan's network predicts %s; the derivative of the x0 / v adapter is not built: an eps network only", what,
                 plan->pred == DMME_PRED_X0 ? "x0" : "v");
    DMME_REQUIRE(plan->thr_mode == DMME_THRESHOLD_NONE, DMME_ERR_UNSUPPORTED,
                 "%s: the plan thresholds x0 (mode %d); the derivative of the clip is not built: threshold none only", what, plan->thr_mode);
    return DMME_OK;
}

// DPS: kind DMME_CHAIN_DPS, which differentiates the denoiser itself: the keep form of the forward, the adjoint kernel (csrc/dps.hip) that
// leaves d ||y - A x0|| / d eps (up to the per-image 1 / ||r||) in d_out, the input-only backward, the update that consumes both
DMME_API int dmme_dps_chain_step(const dmme_plan* plan, const void* packed, const void* packed_bwd, float* x, float* model_out, void* workspace,
                                 void* bwd_workspace, const float* y, const float* mask, const float* Kh, const float* Kw, int h, int w, float* g, float* d_out,
                                 float* dx, float* sumsq, const float* step_coef, const int64_t* t_table, void* state, void* stream) {
    DMME_REQUIRE(plan && packed && packed_bwd && x && model_out && workspace && bwd_workspace && y && Kh && Kw && g && d_out && dx && sumsq && step_coef &&
                     t_table && state,
                 DMME_ERR_INVALID, "dps_chain_step: null argument");
    if (int rc = require_differentiable_plan("dps_chain_step", plan)) return rc;
    int planes = 0;
    if (int rc = chain_step_front("dps_chain_step", plan, packed, x, nullptr, nullptr, model_out, workspace, DMME_CHAIN_DPS, false, 0, nullptr, 8, 0, state, stream,
                                  planes, true))
        return rc;
    const int B = plan->B, C = plan->cfg.in_channels, H = plan->H, W = plan->W;
    if (int rc = launch_dps_adjoint("dps_chain_step", x, model_out, y, mask, Kh, Kw, nullptr, step_coef, state, g, d_out, sumsq, B, C, H, W, h, w, planes,
                                    (hipStream_t)stream))
        return rc;
    const int64_t* t_dev = (const int64_t*)state + 1;
    if (int rc = dmme_unet_backward_input(plan, packed, packed_bwd, x, t_dev, 1, d_out, workspace, bwd_workspace, nullptr, dx, stream)) return rc;
    return launch_dps_update("dps_chain_step", x, model_out, g, dx, sumsq, nullptr, nullptr, step_coef, t_table, state, B, C, H, W, planes, (hipStream_t)stream);
}

// Probability-flow ODE: kind DMME_CHAIN_PFODE, one Heun STAGE per loop index (csrc/pfode.hip).  The sampling / encoding step is the front
// half every chain step has and the four-term stage update; the tables alone say which way the walk goes.
DMME_API int dmme_pf_chain_step(const dmme_plan* plan, const void* packed, float* x, float* model_out, void* workspace, float* xs, float* es,
                                const float* step_coef, const int64_t* t_table, void* state, void* stream) {
    DMME_REQUIRE(plan && packed && x && model_out && workspace && xs && es && step_coef && t_table && state, DMME_ERR_INVALID, "pf_chain_step: null argument");
    int planes = 0;
    if (int rc = chain_step_front("pf_chain_step", plan, packed, x, nullptr, nullptr, model_out, workspace, DMME_CHAIN_PFODE, false, 0, nullptr, 8, 0, state, stream,
                                  planes))
        return rc;
    return launch_pf_stage("pf_chain_step", x, model_out, planes, xs, es, nullptr, step_coef, t_table, state, 0, plan->B,
                           (int64_t)plan->cfg.in_channels * plan->H * plan->W, (hipStream_t)stream);
}

// ... and the likelihood's stage, which differentiates the denoiser as DPS does: the keep form of the forward, the Rademacher probe z
// written as d_out, the input-only backward (dx = J^T z), the probe dot into the per-image double accumulator, the stage update
DMME_API int dmme_pf_ll_chain_step(const dmme_plan* plan, const void* packed, const void* packed_bwd, float* x, float* model_out, void* workspace,
                                   void* bwd_workspace, float* xs, float* es, float* d_out, float* dx, float* scratch, float* s_out, double* acc,
                                   const float* step_coef, const int64_t* t_table, void* state, void* stream) {
    DMME_REQUIRE(plan && packed && packed_bwd && x && model_out && workspace && bwd_workspace && xs && es && d_out && dx && scratch && s_out && acc && step_coef &&
                     t_table && state,
                 DMME_ERR_INVALID, "pf_ll_chain_step: null argument");
    if (int rc = require_differentiable_plan("pf_ll_chain_step", plan)) return rc;
    DMME_REQUIRE(!plan->mix, DMME_ERR_UNSUPPORTED, "pf_ll_chain_step: precision fp16r32 is an inference mode (no backward)");
    int planes = 0;
    if (int rc = chain_step_front("pf_ll_chain_step", plan, packed, x, nullptr, nullptr, model_out, workspace, DMME_CHAIN_PFODE, false, 0, nullptr, 8, 0, state,
                                  stream, planes, true))
        return rc;
    const int B = plan->B;
    const int64_t chw = (int64_t)plan->cfg.in_channels * plan->H * plan->W;
    if (int rc = launch_pf_probe("pf_ll_chain_step", d_out, state, 0, 0, B, chw, planes, (hipStream_t)stream)) return rc;
    const int64_t* t_dev = (const int64_t*)state + 1;
    if (int rc = dmme_unet_backward_input(plan, packed, packed_bwd, x, t_dev, 1, d_out, workspace, bwd_workspace, nullptr, dx, stream)) return rc;
    if (int rc = launch_pf_dot("pf_ll_chain_step", d_out, planes, dx, nullptr, step_coef, state, B, chw, scratch, s_out, acc, (hipStream_t)stream)) return rc;
    return launch_pf_stage("pf_ll_chain_step", x, model_out, planes, xs, es, nullptr, step_coef, t_table, state, 1, B, chw, (hipStream_t)stream);
}

// Dhariwal & Nichol 2021, Algorithm 1 (DDPM) / 2 (DDIM): between the forward and the update, the classifier's forward, the log-softmax
// gradient and the input-only backward leave d log p(y | x_t, t) / d x_t in `grad`
DMME_API int dmme_guided_chain_step(const dmme_plan* plan, const void* packed, const dmme_plan* cls, const void* cls_packed,
                                    const void* cls_packed_bwd, float* x, float* model_out, void* workspace, void* cls_workspace,
                                    void* cls_bwd_workspace, const int64_t* y, float* logits, float* d_logits, float* grad, int* status,
                                    int kind, const float* step_coef, const int64_t* t_table, void* state, void* stream) {
    DMME_REQUIRE(plan && packed && cls && cls_packed && cls_packed_bwd && x && model_out && workspace && cls_workspace && cls_bwd_workspace && y &&
                 logits && d_logits && grad && step_coef && t_table && state, DMME_ERR_INVALID, "guided_chain_step: null argument");
    DMME_REQUIRE(kind_grad(kind), DMME_ERR_INVALID, "guided_chain_step: kind %d is not a guided kind", kind);
    DMME_REQUIRE(plan->cfg.arch == DMME_ARCH_DDPM && !plan->cond && cls->cfg.arch == DMME_ARCH_CLASSIFIER, DMME_ERR_INVALID,
                 "guided_chain_step: needs a DDPM UNet plan and a classifier plan (got architectures %d, %d)", plan->cfg.arch, cls->cfg.arch);
    DMME_REQUIRE(plan->B == cls->B && plan->H == cls->H && plan->W == cls->W && plan->cfg.in_channels == cls->cfg.in_channels, DMME_ERR_INVALID,
                 "guided_chain_step: the UNet plan (B=%d %dx%d) and the classifier plan (B=%d %dx%d) differ", plan->B, plan->H, plan->W, cls->B, cls->H, cls->W);
    const int64_t* t_dev = (const int64_t*)state + 1;
    return chain_step_common("guided_chain_step", plan, packed, x, nullptr, nullptr, model_out, workspace, kind, grad, nullptr, step_coef, t_table, state, stream, [&] {
        int rc = unet_forward_impl(cls, cls_packed, x, t_dev, 1, logits, cls_workspace, nullptr, stream, true);
        if (rc == DMME_OK) rc = launch_log_softmax_grad(logits, y, cls->B, cls->out_channels, 1, 1.0f, nullptr, d_logits, status, (hipStream_t)stream);
        if (rc == DMME_OK)
            rc = dmme_unet_backward_input(cls, cls_packed, cls_packed_bwd, x, t_dev, 1, d_logits, cls_workspace, cls_bwd_workspace, nullptr, grad, stream);
        return rc;
    });
}

DMME_API int dmme_label_dropout(const int64_t* labels, int B, int K, float p, uint64_t seed, uint64_t offset, int64_t* out, int* status, void* stream) {
    return launch_label_dropout(labels, B, K, p, seed, offset, out, status, (hipStream_t)stream);
}

// The two launches of dmme_slerp hand three partial sums per (image, block) from one to the other.  The entry point takes no scratch
// argument, so the library keeps one buffer per device, grown on demand (hipFree waits for the device: no launch still reads the old one).
DMME_API int dmme_slerp(const float* xa, const float* xb, const float* w, int n, int B, int64_t chw, float* out, void* stream) {
    DMME_REQUIRE(xa && xb && w && out, DMME_ERR_INVALID, "slerp: null argument");
    DMME_REQUIRE(n > 0 && B > 0 && B <= 65535 && chw > 0, DMME_ERR_INVALID, "slerp: n = %d weights, B = %d images of %lld values", n, B, (long long)chw);
    DMME_REQUIRE(chw % 4 == 0, DMME_ERR_INVALID, "slerp: image size %lld is not a multiple of 4", (long long)chw);
    static std::mutex mu;
    static std::map<int, std::pair<float*, size_t>> scratch;  // device -> (buffer, floats)
    const size_t need = (size_t)3 * B * slerp_parts(chw);
    float* buf = nullptr;
    {
        std::lock_guard<std::mutex> lock(mu);
        int dev = 0;
        DMME_CHECK_HIP(hipGetDevice(&dev));
        auto& e = scratch[dev];
        if (e.second < need) {
            if (e.first) DMME_CHECK_HIP(hipFree(e.first));
            e = {nullptr, 0};
            const size_t cap = need < 4096 ? 4096 : need;
            DMME_CHECK_HIP(hipMalloc((void**)&e.first, cap * sizeof(float)));
            e.second = cap;
        }
        buf = e.first;
    }
    return launch_slerp(xa, xb, w, n, B, chw, out, buf, (hipStream_t)stream);
}

DMME_API int dmme_log_softmax_grad(const float* logits, const int64_t* y, int B, int K, int mode, float scale, float* loss, float* d_logits,
                                   int* status, void* stream) {
    return launch_log_softmax_grad(logits, y, B, K, mode, scale, loss, d_logits, status, (hipStream_t)stream);
}

DMME_API int dmme_image_batch(const uint8_t* data, int64_t n_images, const int64_t* idx, const uint8_t* flip, int B, int C, int H, int W,
                              float* out, void* stream) {
    DMME_REQUIRE(data && idx && out && n_images > 0 && B > 0 && C > 0 && H > 0 && W > 0, DMME_ERR_INVALID, "image_batch: bad argument");
    return launch_image_batch(data, idx, flip, B, C, H, W, out, (hipStream_t)stream);
}

DMME_API int dmme_grid_tile(const float* x, int B, int C, int H, int W, int cell0, int cell_stride, int xmaps, int ymaps, int pad, int out_kind, int raw,
                            void* canvas, void* stream) {
    DMME_REQUIRE(x && canvas, DMME_ERR_INVALID, "grid_tile: null pointer");
    DMME_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0 && xmaps > 0 && ymaps > 0 && pad >= 0, DMME_ERR_INVALID,
                 "grid_tile: %d images of %d x %d x %d into %d x %d cells, padding %d", B, C, H, W, ymaps, xmaps, pad);
    DMME_REQUIRE(cell0 >= 0 && cell_stride >= 1 && cell0 + (int64_t)(B - 1) * cell_stride < (int64_t)xmaps * ymaps, DMME_ERR_INVALID,
                 "grid_tile: cells %d + b * %d of %d images do not fit a grid of %d x %d", cell0, cell_stride, B, ymaps, xmaps);
    DMME_REQUIRE(out_kind == 0 || out_kind == 1, DMME_ERR_INVALID, "grid_tile: out_kind %d (0: float32, 1: uint8)", out_kind);
    DMME_REQUIRE(raw == 0 || raw == 1, DMME_ERR_INVALID, "grid_tile: raw %d (0: denorm, 1: the values as they are)", raw);
    return launch_grid_tile(x, B, C, H, W, cell0, cell_stride, xmaps, ymaps, pad, out_kind, raw, canvas, (hipStream_t)stream);
}

DMME_API int dmme_iddpm_loss(const float* model_out, const float* x_t, const float* x_0, const float* target, const int64_t* t,
                             const float* coef, int B, int64_t chw, float w_simple, float w_vlb, float* loss, float* d_out,
                             float grad_scale, float* scratch, void* stream) {
    DMME_REQUIRE(model_out && x_t && x_0 && target && t && coef && loss && scratch && B > 0 && chw > 0, DMME_ERR_INVALID,
                 "iddpm_loss: bad argument");
    return launch_iddpm_loss(model_out, x_t, x_0, target, t, coef, B, chw, w_simple, w_vlb, loss, d_out, grad_scale, scratch,
                             (hipStream_t)stream);
}

DMME_API int dmme_iddpm_loss_rows(const float* model_out, const float* x_t, const float* x_0, const float* target, const int64_t* t,
                                  const float* coef, int T, const float* weight, int B, int64_t chw, float w_simple, float w_vlb, float* loss,
                                  float* rows, float* d_out, float grad_scale, int* status, float* scratch, void* stream) {
    return launch_iddpm_loss_rows(model_out, x_t, x_0, target, t, coef, T, weight, B, chw, w_simple, w_vlb, loss, rows, d_out, grad_scale, status,
                                  scratch, (hipStream_t)stream);
}

DMME_API int dmme_iddpm_prior_rows(const float* x_0, int B, int64_t chw, float alpha_bar_T, float* prior, void* stream) {
    return launch_iddpm_prior_rows(x_0, B, chw, alpha_bar_T, prior, (hipStream_t)stream);
}

DMME_API int dmme_tsampler_draw(const float* hist, const int* count, int T, int H, float uniform_prob, uint64_t philox_seed,
                                uint64_t philox_offset, int B, int64_t* t, float* weight, float* p, void* stream) {
    return launch_tsampler_draw(hist, count, T, H, uniform_prob, philox_seed, philox_offset, B, t, weight, p, (hipStream_t)stream);
}

DMME_API int dmme_tsampler_update(float* hist, int* count, int T, int H, const int64_t* t, const float* L, int B, int* status, void* stream) {
    return launch_tsampler_update(hist, count, T, H, t, L, B, status, (hipStream_t)stream);
}

DMME_API int dmme_mse_loss(const float* eps, const float* target, int64_t numel, float* loss, float* d_eps, float grad_scale,
                  float* scratch, void* stream) {
    DMME_REQUIRE(eps && target && loss && scratch, DMME_ERR_INVALID, "mse_loss: null argument");
    return launch_mse(eps, target, numel, loss, d_eps, grad_scale, scratch, (hipStream_t)stream);
}

DMME_API int dmme_debug_issue_probe(int kind, int n_inner, int iters, int flags, int blocks, void* sink, const void* src, void* stream) {
    return launch_issue_probe(kind, n_inner, iters, flags, blocks, (long long*)sink, src, (hipStream_t)stream);
}
DMME_API int dmme_debug_mfma_valu(int mode, int iters, int blocks, void* sink, void* stream) {
    DMME_REQUIRE(sink && iters > 0 && blocks > 0, DMME_ERR_INVALID, "mfma_valu: bad argument");
    return launch_mfma_valu(mode, iters, blocks, (float*)sink, (hipStream_t)stream);
}
DMME_API int dmme_debug_l2_stream(const void* buf, int64_t bytes, int iters, int mode, int depth, int blocks, void* sink, void* stream) {
    return launch_l2_stream(buf, bytes, iters, mode, depth, blocks, (unsigned*)sink, (hipStream_t)stream);
}

static long long* g_stamps = nullptr;
DMME_API int dmme_debug_set_stamps(void* buf) {
    g_stamps = (long long*)buf;
    return DMME_OK;
}

DMME_API int dmme_conv2d(const dmme_conv_desc* d, const void* src1, const void* src2, const void* weight, const float* bias,
                const float* scale, const float* shift, const float* dmask, const float* tproj, const void* res1,
                const void* res2, int R1, void* dst, void* stream) {
    DMME_REQUIRE(d && src1 && weight && bias && dst, DMME_ERR_INVALID, "conv2d: null argument");
    DMME_REQUIRE(d->taps == 9 || d->taps == 1, DMME_ERR_INVALID, "conv2d: taps must be 1 or 9");
    DMME_REQUIRE(d->stride == 1 || d->stride == 2, DMME_ERR_INVALID, "conv2d: stride must be 1 or 2");
    ConvArgs a{};
    a.src1 = src1; a.src2 = src2; a.w = weight; a.bias = bias; a.scale = scale; a.shift = shift; a.dmask = dmask;
    a.tproj = d->nt > 0 ? tproj : nullptr;
    a.res1 = res1; a.res2 = res2; a.R1 = R1; a.dst = dst;
    a.N = d->N; a.Hin = d->Hin; a.Win = d->Win; a.C1 = d->C1; a.C2 = src2 ? d->C2 : 0;
    a.up = d->upsample; a.stride = d->stride; a.taps = d->taps;
    const int Hv = a.up ? 2 * a.Hin : a.Hin, Wv = a.up ? 2 * a.Win : a.Win;
    a.Hout = Hv / a.stride; a.Wout = Wv / a.stride; a.Cout = d->Cout;
    a.pro_silu = d->pro_silu; a.out_silu = d->out_silu; a.nt = d->nt; a.tproj_ld = d->tproj_ld;
    a.in_nchw = d->in_nchw; a.out_nchw = d->out_nchw;
    a.stamps = g_stamps;
    DMME_REQUIRE(d->dtype == DMME_F32 || d->dtype == DMME_BF16 || d->dtype == DMME_BF16X3 || d->dtype == DMME_F16 || d->dtype == DMME_F16R32, DMME_ERR_INVALID,
                 "conv2d: bad dtype %d", d->dtype);
    a.x3 = d->dtype == DMME_BF16X3;
    a.f16 = d->dtype == DMME_F16;
    if (d->dtype == DMME_F16R32) {
        // the split-pass kernels of the mixed mode's fp32 level, as single ops: fp32 tensors (NHWC; the thin output conv writes NCHW),
        // filter packed by dmme_pack_weight(DMME_F16R32): [Cout][taps][Cin / 32][hi 32 | lo 32] halves.  No fall-back to other kernels.
        a.mix = a.out_nchw ? 3 : a.taps == 1 ? 4 : 1;
        a.f16 = 1;
        const ConvRoute r = conv_route(DMME_F16, a);
        DMME_REQUIRE(r.family == (a.mix == 4 ? CONV1X1_SPLIT : a.mix == 3 ? CONV_THIN : CONV3X3_SPLIT), DMME_ERR_UNSUPPORTED, "conv2d(fp16r32): the %s does not take this shape",
                     a.mix == 4 ? "split-pass 1x1 kernel" : a.mix == 3 ? "thin output conv" : "split-pass 3x3 kernel");
        return launch_conv(r, DMME_F16, a, (hipStream_t)stream);
    }
    return launch_conv(a.x3 ? DMME_F32 : d->dtype, a, (hipStream_t)stream, d->force_generic);
}

DMME_API int dmme_conv2d_res(const dmme_conv_desc* d, const void* src1, const void* src2, const void* weight, const float* bias, const float* scale,
                             const float* shift, const float* dmask, const void* r_src1, const void* r_src2, int r_C1, int r_C2, const void* r_weight,
                             const float* r_bias, void* dst, void* stream) {
    DMME_REQUIRE(d && src1 && weight && bias && dst && r_src1 && r_weight && r_bias, DMME_ERR_INVALID, "conv2d_res: null argument");
    DMME_REQUIRE(d->dtype == DMME_BF16 || d->dtype == DMME_F16, DMME_ERR_UNSUPPORTED, "conv2d_res: 16-bit tensors only (dtype %d)", d->dtype);
    ConvArgs a{};
    a.src1 = src1; a.src2 = src2; a.w = weight; a.bias = bias; a.scale = scale; a.shift = shift; a.dmask = dmask; a.dst = dst;
    a.N = d->N; a.Hin = d->Hin; a.Win = d->Win; a.C1 = d->C1; a.C2 = src2 ? d->C2 : 0;
    a.up = d->upsample; a.stride = d->stride; a.taps = d->taps;
    a.Hout = a.Hin; a.Wout = a.Win; a.Cout = d->Cout;
    a.pro_silu = d->pro_silu; a.out_silu = d->out_silu;
    a.f16 = d->dtype == DMME_F16;
    a.stamps = g_stamps;
    a.r_src1 = r_src1; a.r_src2 = r_C2 > 0 ? r_src2 : nullptr; a.r_C1 = r_C1; a.r_C2 = r_C2 > 0 ? r_C2 : 0; a.r_w = r_weight; a.r_bias = r_bias;
    const ConvRoute r = conv_route(d->dtype, a);
    DMME_REQUIRE(a.taps == 9 && a.stride == 1 && !a.up && r.rseg, DMME_ERR_UNSUPPORTED,
                 "conv2d_res: the wave-specialised 3x3 kernel does not take this shape with a residual segment (%d+%d -> %d channels, %d+%d raw, %dx%dx%d)", a.C1, a.C2,
                 a.Cout, a.r_C1, a.r_C2, a.N, a.Hin, a.Win);
    return launch_conv(r, d->dtype, a, (hipStream_t)stream);
}

DMME_API int dmme_groupnorm_scale_shift(int dtype, const void* src1, const void* src2, int N, int HW, int C1, int C2, int groups,
                               const float* gamma, const float* beta, float eps, float* scale, float* shift,
                               float* partial_scratch, int force_generic, void* stream) {
    DMME_REQUIRE(src1 && gamma && beta && scale && shift, DMME_ERR_INVALID, "groupnorm: null argument");
    if (!src2) C2 = 0;
    DMME_REQUIRE(groups > 0 && (C1 + C2) % groups == 0, DMME_ERR_INVALID, "groupnorm: %d channels not divisible by %d groups",
                 C1 + C2, groups);
    if (!force_generic && partial_scratch && gn_fast_supported(dtype, N, HW, C1, C2, groups))
        return launch_gn_fast(dtype, src1, src2, N, HW, C1, C2, groups, gamma, beta, eps, scale, shift, nullptr,
                              partial_scratch, (hipStream_t)stream);
    return launch_gn_generic(dtype, src1, src2, N, HW, C1, C2, groups, gamma, beta, eps, scale, shift, nullptr,
                             (hipStream_t)stream);
}

DMME_API int dmme_attention(int dtype, const void* qkv, int N, int S, int C, void* out, int force_generic, void* stream) {
    DMME_REQUIRE(qkv && out && N > 0 && S > 0 && C > 0, DMME_ERR_INVALID, "attention: bad argument");
    if (dtype == DMME_BF16X3) {  // fp32 buffers; the three-pass MFMA kernel where it applies
        if (!force_generic && attn_x3_supported(N, S, C, 1)) return launch_attn_x3(qkv, N, S, C, 1, out, (hipStream_t)stream);
        dtype = DMME_F32;
    }
    if (!force_generic && attn_mfma_supported(dtype, N, S, C)) return launch_attn_mfma(dtype, qkv, N, S, C, out, nullptr, (hipStream_t)stream);
    return launch_attn_generic(dtype, qkv, N, S, C, out, (hipStream_t)stream);
}

DMME_API int dmme_attention_proj(int dtype, const void* qkv, int N, int S, int C, const void* w, const float* bias, const void* res, void* dst, void* ctx,
                                 float* gn_part, int gn_cg, void* stream) {
    DMME_REQUIRE(qkv && w && bias && res && dst && N > 0 && S > 0 && C > 0, DMME_ERR_INVALID, "attention_proj: bad argument");
    return launch_attn_proj(dtype, qkv, N, S, C, ctx, nullptr, w, bias, res, dst, gn_part, S / 32, gn_cg, (hipStream_t)stream, g_stamps);
}

// one folded block as a single op (attn_mfma.hip, AttnFold): the fold of its weights, then the launch
DMME_API int dmme_attention_fold(int dtype, int C, const void* wqkv, const float* bqkv, const void* wp, const float* bp, void* M, float* c, void* wpv, float* bias2,
                                 void* stream) {
    DMME_REQUIRE(wqkv && bqkv && wp && bp && M && c && wpv && bias2 && C > 0, DMME_ERR_INVALID, "attention_fold: bad argument");
    AttnFoldJob jb{};  // byte offsets from a null base: the addresses themselves
    jb.wq = (int64_t)(intptr_t)wqkv;
    jb.bq = (int64_t)(intptr_t)bqkv;
    jb.wp = (int64_t)(intptr_t)wp;
    jb.bp = (int64_t)(intptr_t)bp;
    jb.M = (int64_t)(intptr_t)M;
    jb.c = (int64_t)(intptr_t)c;
    jb.wpv = (int64_t)(intptr_t)wpv;
    jb.bias2 = (int64_t)(intptr_t)bias2;
    jb.C = C;
    return launch_attn_fold_weights(dtype, nullptr, 1, C, nullptr, (hipStream_t)stream, &jb);
}
DMME_API int dmme_attention_block(int dtype, const void* x, int N, int S, int C, const float* parts, int part_tiles, int part_cnt, int groups, const float* gamma,
                                  const float* beta, float eps, float* scale, float* shift, const void* M, const float* c, const void* wpv, const float* bias2,
                                  const void* res, void* dst, float* gn_part, int gn_cg, void* stream) {
    DMME_REQUIRE(x && M && c && wpv && bias2 && res && dst && N > 0 && S > 0 && C > 0, DMME_ERR_INVALID, "attention_block: bad argument");
    GnIn gni{};
    if (parts) {  // the norm finished inside the launch from [N][part_tiles][groups] {mean, M2} partials of part_cnt elements each
        DMME_REQUIRE(gamma && beta && groups > 0 && part_tiles > 0 && part_cnt > 0, DMME_ERR_INVALID, "attention_block: partials without gamma / beta / geometry");
        gni.p1 = parts;
        gni.t1 = part_tiles;
        gni.cnt1 = part_cnt;
        gni.C1 = C;
        gni.groups = groups;
        gni.gamma = gamma;
        gni.beta = beta;
        gni.eps = eps;
    }
    return launch_attn_fold(dtype, x, N, S, C, parts ? &gni : nullptr, scale, shift, M, c, wpv, bias2, res, dst, gn_part, S / 32, gn_cg, (hipStream_t)stream, g_stamps);
}

DMME_API int dmme_attention_heads(int dtype, const void* qkv, int N, int S, int C, int heads, void* out, int force_generic, void* stream) {
    DMME_REQUIRE(qkv && out && N > 0 && S > 0 && C > 0 && heads > 0 && C % heads == 0, DMME_ERR_INVALID, "attention_heads: bad argument");
    if (dtype == DMME_BF16X3) {
        if (!force_generic && attn_x3_supported(N, S, C, heads)) return launch_attn_x3(qkv, N, S, C, heads, out, (hipStream_t)stream);
        dtype = DMME_F32;
    }
    if (!force_generic && attn_heads_mfma_supported(dtype, N, S, C, heads))
        return launch_attn_heads_mfma(dtype, qkv, N, S, C, heads, out, nullptr, (hipStream_t)stream);
    return launch_attn_heads(dtype, qkv, N, S, C, heads, out, (hipStream_t)stream);
}

DMME_API int dmme_nchw_to_nhwc(int dtype, const float* src, int N, int C, int HW, void* dst, void* stream) {
    DMME_REQUIRE(src && dst, DMME_ERR_INVALID, "nchw_to_nhwc: null argument");
    return launch_nchw_to_nhwc(dtype, src, N, C, HW, dst, (hipStream_t)stream);
}
DMME_API int dmme_nhwc_to_nchw(int dtype, const void* src, int N, int C, int HW, float* dst, void* stream) {
    DMME_REQUIRE(src && dst, DMME_ERR_INVALID, "nhwc_to_nchw: null argument");
    return launch_nhwc_to_nchw(dtype, src, N, C, HW, dst, (hipStream_t)stream);
}
DMME_API int dmme_pack_weight(int dtype, const float* src, int Cout, int Cin, int taps, void* dst, void* stream) {
    DMME_REQUIRE(src && dst, DMME_ERR_INVALID, "pack_weight: null argument");
    return launch_pack_weight(dtype, src, Cout, Cin, taps, dst, (hipStream_t)stream);
}

DMME_API int dmme_event_create(void** ev) {
    DMME_REQUIRE(ev, DMME_ERR_INVALID, "event_create: null");
    hipEvent_t e;
    DMME_CHECK_HIP(hipEventCreate(&e));
    *ev = (void*)e;
    return DMME_OK;
}
DMME_API int dmme_event_record(void* ev, void* stream) {
    DMME_CHECK_HIP(hipEventRecord((hipEvent_t)ev, (hipStream_t)stream));
    return DMME_OK;
}
DMME_API int dmme_event_elapsed_ms(void* start, void* stop, float* ms) {
    DMME_CHECK_HIP(hipEventSynchronize((hipEvent_t)stop));
    DMME_CHECK_HIP(hipEventElapsedTime(ms, (hipEvent_t)start, (hipEvent_t)stop));
    return DMME_OK;
}
DMME_API int dmme_event_destroy(void* ev) {
    DMME_CHECK_HIP(hipEventDestroy((hipEvent_t)ev));
    return DMME_OK;
}

}  // extern "C"
