// Backward side of the plan.  Planning (plan_backward, host arithmetic, in named phases): the workspace layout, gradient buckets for the
// overlapped data-parallel exchange, the grouped weight-gradient tables, the deferred bias / column-sum jobs, the tiled time-projection
// gradient.  Execution: the per-op routes (attn_bwd_route, bias_route, wgrad_route; the GroupNorm's is bwd_fast.hip's gn_bwd_route, the
// data gradient's conv_route on dgrad_args), and the reverse walk over the op list in steps (BwdRun).
#include "plan.h"

using namespace dmme;

namespace dmme {

// The route of the GroupNorm backward in front of conv o (o.gn >= 0), at the plan's real batch: the one question the layout, the
// deferred tables and the walk ask
static GnBwdRoute gn_route_of(const dmme_plan* P, const Op& o) {
    const Op& gop = P->ops[o.gn];
    const Tensor& t1 = P->tensors[gop.gn_src1];
    return gn_bwd_route(P->dtype, P->B, t1.H * t1.W, t1.C, gop.gn_src2 >= 0 ? P->tensors[gop.gn_src2].C : 0, P->cfg.num_groups, gop.gn_mod_col >= 0);
}

// Backward workspace: one gradient buffer per forward tensor (shared where the plan aliases them), the region cleared once per backward,
// per-op scratch, temporaries.  build_wgrad_group appends the activated tensors of the grouped weight gradient behind it.
static void layout_backward(dmme_plan* P) {
    const dmme_unet_cfg& c = P->cfg;
    std::vector<Op>& ops = P->ops;
    const int B = P->B, tcols = P->tproj_cols;
    const int64_t es = (int64_t)dtype_size(P->dtype);
    const bool cls = c.arch == DMME_ARCH_CLASSIFIER;
    int64_t bw = 0;
    auto balloc = [&](int64_t bytes) {
        const int64_t o = bw;
        bw = align_up(bw + bytes, 256);
        return o;
    };
    int64_t tmp_max = 0, att_max = 0;
    int cmax = c.in_channels;
    for (const Tensor& t : P->tensors) {
        P->gt_off.push_back(balloc((int64_t)B * t.H * t.W * t.C * es));
        if (t.C > cmax) cmax = t.C;
    }
    // A ResBlock's 1x1 residual conv feeds nothing but the residual input of conv2: the gradient of its output IS the gradient of
    // the block's output - the two tensors share one gradient buffer instead of a copy launch per block
    if (!debug_route("no_res_alias")) {
        std::vector<int> uses(P->tensors.size(), 0), producer(P->tensors.size(), -1);
        for (int oi = 0; oi < (int)ops.size(); ++oi) {
            const Op& o = ops[oi];
            for (int id : {o.src1, o.src2, o.res1, o.res2, o.gn_src1, o.gn_src2, o.at_qkv})
                if (id >= 0) ++uses[id];
            if (o.kind == OP_CONV && o.dst >= 0) producer[o.dst] = oi;
        }
        for (Op& o : ops) {
            if (o.kind != OP_CONV || o.res1 < 0 || o.res2 >= 0 || o.dst < 0) continue;
            const int r = o.res1;
            if (uses[r] != 1 || producer[r] < 0 || ops[producer[r]].kind != OP_CONV || P->tensors[r].C != P->tensors[o.dst].C) continue;
            P->gt_off[r] = P->gt_off[o.dst];
            o.res_alias = 1;
        }
    }
    for (const Op& o : ops) {
        if (o.kind == OP_CONV && o.src1 >= 0) {
            const Tensor& t1 = P->tensors[o.src1];
            const int Cin = t1.C + (o.src2 >= 0 ? P->tensors[o.src2].C : 0);
            const int64_t up = o.up ? 4 : 1;
            const int64_t b = (int64_t)B * t1.H * t1.W * up * Cin * es;
            if (b > tmp_max) tmp_max = b;
        }
        if (o.kind == OP_ATTN) {
            const Tensor& q = P->tensors[o.at_qkv];
            const int64_t b = (int64_t)B * o.at_heads * q.H * q.W * q.H * q.W * 4;
            if (b > att_max) att_max = b;
        }
    }
    {   // accumulation scratch, one contiguous region cleared by a single memset per backward:
        // packed-layout weight-gradient image, per-conv column sums, per-GroupNorm channel sums
        P->bws_zero = bw;
        int64_t wfl = 0;
        for (Param& p : P->params)
            if (p.ndim == 4) {
                p.wp_off = wfl;
                wfl += (p.numel() + 63) / 64 * 64;
            }
        P->bws_wimage = balloc(wfl * 4);
        for (Op& o : P->ops) {
            if (o.kind != OP_CONV) continue;
            o.b_rowsum = balloc((int64_t)B * P->params[o.w].cout * 4);
        }
        P->bws_zpage = balloc(256);  // a page of zeros: the padding rows of the DMA-fed weight gradient
        P->bws_zero_bytes = bw - P->bws_zero;
        for (Op& o : P->ops) {  // GroupNorm channel sums, one partial row per pixel chunk (written whole: outside the cleared region)
            if (o.kind != OP_CONV || o.gn < 0) continue;
            const Op& gop = P->ops[o.gn];
            const Tensor& t1 = P->tensors[gop.gn_src1];
            const int C = t1.C + (gop.gn_src2 >= 0 ? P->tensors[gop.gn_src2].C : 0);
            o.b_ab = balloc((int64_t)gn_route_of(P, o).nchunks * B * C * 2 * 4);
            o.b_gnrows = balloc((int64_t)2 * B * C * 4);
        }
        P->bws_gnS = balloc((int64_t)B * c.num_groups * 2 * 4);
    }
    P->sink_half = (int64_t)2 * cmax;  // (a concatenated GroupNorm input has up to 2 x the widest tensor's channels)
    P->bws_sink = balloc(2 * P->sink_half * 4);
    if (cls) {
        P->bws_hpool = balloc((int64_t)B * P->tensors[P->head_src].C * 4);
        P->bws_hrows = balloc((int64_t)B * 2 * P->tensors[P->head_src].C * 4);
    }
    P->bws_tmp = balloc(tmp_max);
    P->bws_dy = balloc(cls ? (int64_t)B * P->out_channels * 4 : (int64_t)B * P->H * P->W * P->out_channels * es);  // (classifier: d logits, fp32)
    P->bws_rowsum = balloc((int64_t)B * cmax * 3 * 4);  // qkv convs have 3*C outputs
    P->bws_dtproj = balloc((int64_t)B * tcols * 4);
    P->bws_dtemb = balloc((int64_t)B * c.emb_dim * 4);
    P->bws_dh1 = balloc((int64_t)B * c.emb_dim * 4);
    P->bws_z = balloc((int64_t)B * c.emb_dim * 4);
    P->bws_wT = balloc((int64_t)(tcols > c.emb_dim ? tcols : c.emb_dim) * c.emb_dim * es);
    P->bws_attP = balloc(att_max);
    P->bws_attdS = balloc(att_max);
    P->bws_bytes = bw;
}

// Grouped weight gradients: every 3x3 stride-1 conv the all-taps MFMA kernel supports is taken out of the per-layer
// sequence; its (cout tile, cin tile) pairs are cut into jobs of at most `q` consecutive 64-pixel tiles, longest first.
static void build_wgrad_group(dmme_plan* P, dmme_plan::WgGroup& G, int gi, int op_lo = 0, int op_hi = 1 << 30) {
    const int taps = gi == 1 ? 1 : 9, stride = gi == 2 ? 2 : 1;
    G.taps = taps;
    G.stride = stride;
    if (stride == 2 && debug_route("no_wg_s2")) return;
    if (!is16(P->dtype) || getenv("DMME_NO_WGRAD_GROUP")) return;
    // (the stride-2 table is three small layers: shorter jobs, or 80 workgroups would carry it)
    const int q = stride == 2 ? 16 : 64;
    struct Grp { int layer, n_co, n_ci, tile0, ntiles; };
    std::vector<Grp> groups;
    for (int oi = (int)P->ops.size() - 1; oi >= 0; --oi) {
        Op& o = P->ops[oi];
        if (o.kind != OP_CONV || o.src1 < 0 || o.dst < 0 || o.taps != taps || o.stride != stride || oi < op_lo || oi >= op_hi) continue;
        ConvArgs a{};
        fill_conv(P, o, nullptr, nullptr, nullptr, nullptr, nullptr, 1, a);
        WgLayer L{};
        int CO = 0, CI = 0;
        if (!wgrad_mfma_supported(P->dtype, a) || !wgrad_group_layer(P->dtype, a, L, &CO, &CI)) continue;
        L.src1_off = P->tensors[o.src1].off;
        L.src2_off = o.src2 >= 0 ? P->tensors[o.src2].off : -1;
        L.scale_off = o.gn >= 0 ? P->ops[o.gn].gn_scale : -1;
        L.shift_off = o.gn >= 0 ? P->ops[o.gn].gn_shift : -1;
        L.dmask_off = o.dmask_off;
        // The weight gradient's second operand is the conv's ACTIVATED input.  Recomputing GroupNorm + SiLU + dropout per MFMA operand
        // made the grouped kernel VALU-issue bound; instead it reads the activated tensor: the forward's own (small maps, use_act), or
        // one the GroupNorm backward of this conv writes on its way (it holds x, scale, shift and the mask anyway: one more store).
        L.act_off = -1;
        L.act_bws = 0;
        if (o.gn >= 0 && !debug_route("no_wg_act")) {
            const Op& gop = P->ops[o.gn];
            if (o.use_act && gop.gn_act >= 0) {
                L.act_off = gop.gn_act;
            } else if (gop.gn_src1 == o.src1 && gop.gn_src2 == o.src2 && gn_route_of(P, o).writes_act) {
                if (o.wg_act < 0) {
                    o.wg_act = align_up(P->bws_bytes, 256);
                    P->bws_bytes = o.wg_act + (int64_t)P->B * a.Hin * a.Win * (a.C1 + a.C2) * (int64_t)dtype_size(P->dtype);
                }
                L.act_off = o.wg_act;
                L.act_bws = 1;
            }
        }
        L.dy_off = P->gt_off[o.dst];
        L.dw_off = P->params[o.w].wp_off;
        o.wg_layer = (int)G.layers.size();
        G.layers.push_back(L);
        const int n_co = (L.Cout + CO - 1) / CO, n_ci = (L.C1 + L.C2) / CI;
        const int ns = (L.g.tiles_m + q - 1) / q;
        for (int sp = 0; sp < ns; ++sp) {
            Grp gr{};
            gr.layer = o.wg_layer;
            gr.n_co = n_co;
            gr.n_ci = n_ci;
            gr.tile0 = (int)((int64_t)L.g.tiles_m * sp / ns);
            gr.ntiles = (int)((int64_t)L.g.tiles_m * (sp + 1) / ns) - gr.tile0;
            if (gr.ntiles > 0) groups.push_back(gr);
        }
    }
    G.dma = !G.layers.empty() && !debug_route("no_wg_dma");
    for (const WgLayer& L : G.layers)
        if (!(L.act_off >= 0 || ((L.C2 == 0 || taps == 1) && L.scale_off < 0 && L.dmask_off < 0 && !L.pro_silu)) || L.Cout % (taps == 9 ? 64 : 128) ||
            (taps == 1 && (L.C1 + L.C2) % 128))
            G.dma = 0;
    if (stride == 2) {
        if (!G.dma) {  // no register-staged fallback for stride 2: those layers stay on the per-layer kernel
            for (Op& o : P->ops)
                if (o.kind == OP_CONV && o.taps == 9 && o.stride == 2) o.wg_layer = -1;
            G.layers.clear();
            return;
        }
        G.dma = 2;
    }
    // All (cout tile, cin tile) jobs of one pixel range read the same dY and activation tiles: they go to ONE XCD
    // (consecutive positions of its round-robin slice of the grid, blockIdx % 8), so the re-reads hit that XCD's L2
    // instead of HBM.  Groups are placed longest first on the least-loaded XCD; short slices are padded with empty jobs.
    std::stable_sort(groups.begin(), groups.end(), [](const Grp& x, const Grp& y) { return x.ntiles > y.ntiles; });
    const int NX = 8;
    std::vector<WgJob> lists[NX];
    int64_t load[NX] = {0};
    for (const Grp& gr : groups) {
        int best = 0;
        for (int x = 1; x < NX; ++x)
            if (load[x] < load[best]) best = x;
        for (int cot = 0; cot < gr.n_co; ++cot)
            for (int cit = 0; cit < gr.n_ci; ++cit) {
                WgJob j{};
                j.layer = gr.layer;
                j.cot = cot;
                j.cit = cit;
                j.tile0 = gr.tile0;
                j.ntiles = gr.ntiles;
                lists[best].push_back(j);
            }
        load[best] += (int64_t)gr.ntiles * gr.n_co * gr.n_ci;
    }
    size_t longest = 0;
    for (int x = 0; x < NX; ++x) longest = std::max(longest, lists[x].size());
    for (size_t pos = 0; pos < longest; ++pos)
        for (int x = 0; x < NX; ++x) {
            WgJob j{};
            if (pos < lists[x].size()) j = lists[x][pos];
            G.jobs.push_back(j);
        }
}

// Gradient buckets: the op list cut at ResBlock starts, walked in backward order (dmme_plan::GradBucket).  Leaves P->gb empty where
// there is no clean cut.
static void plan_grad_buckets(dmme_plan* P) {
    if (getenv("DMME_NO_GRAD_BUCKETS") || P->cfg.arch == DMME_ARCH_CLASSIFIER) return;  // (the classifier's gradients are not exchanged)
    const int nO = (int)P->ops.size();
    std::vector<int> owner(P->params.size(), -1);  // op index that produces each parameter's gradient (-1: the time MLP, at the very end)
    for (int oi = 0; oi < nO; ++oi) {
        const Op& o = P->ops[oi];
        if (o.kind == OP_CONV) {
            owner[o.w] = oi;
            owner[o.b] = oi;
        } else if (o.kind == OP_GN) {
            owner[o.gn_gamma] = oi;
            owner[o.gn_beta] = oi;
        }
    }
    std::vector<int> tcol_owner(P->tblocks.size(), -1);
    for (size_t k = 0; k < P->tblocks.size(); ++k) {
        const auto& tb = P->tblocks[k];
        for (int oi = 0; oi < nO; ++oi) {
            const Op& o = P->ops[oi];
            if ((o.kind == OP_CONV && o.tproj_col == tb.col) || (o.kind == OP_GN && o.gn_mod_col == tb.col)) tcol_owner[k] = oi;
        }
        if (tcol_owner[k] < 0) return;  // a time projection nothing reads: no clean cut
        owner[tb.tw] = owner[tb.tb] = tcol_owner[k];
    }
    int64_t total = 0;
    for (const Param& p : P->params)
        if (!p.is_buffer) total += p.numel();
    // A block starts at the GroupNorm in front of its conv1.  DDPM: conv1 is the conv that carries the time projection.  IDDPM: conv1
    // is the conv that the modulated (scale-shift) GroupNorm follows directly.
    std::vector<char> is_start(nO, 0);
    for (int oi = 0; oi < nO; ++oi) {
        const Op& o = P->ops[oi];
        if (o.kind != OP_CONV || o.gn < 0) continue;
        const bool conv1 = P->cfg.arch == DMME_ARCH_IDDPM ? (oi + 1 < nO && P->ops[oi + 1].kind == OP_GN && P->ops[oi + 1].gn_mod_col >= 0) : o.tproj_col >= 0;
        if (conv1) is_start[o.gn] = 1;
    }
    const int n_target = debug_route("grad_buckets", 6);
    // candidates: block starts with the fraction of the parameters backward has finished when the walk reaches them
    std::vector<std::pair<int, double>> cand;
    int64_t acc = 0;
    for (int oi = nO - 1; oi > 0; --oi) {
        for (size_t pi = 0; pi < P->params.size(); ++pi)
            if (owner[pi] == oi && !P->params[pi].is_buffer) acc += P->params[pi].numel();
        if (is_start[oi]) cand.push_back({oi, (double)acc / (double)(total > 0 ? total : 1)});
    }
    std::vector<int> cuts{nO};
    if (n_target > 1 && !cand.empty()) {
        // the last cut first: what is left behind it (first down blocks, input conv, time MLP) is the one exchange no compute
        // hides - as close to 12 % of the bytes as the block boundaries allow
        int last = -1;
        double best = 1e9;
        for (int k = 0; k < (int)cand.size(); ++k) {
            const double rest = 1.0 - cand[k].second;
            if (rest < 0.04) continue;
            const double d = rest > 0.12 ? rest - 0.12 : 2.0 * (0.12 - rest);
            if (d < best) { best = d; last = k; }
        }
        if (last >= 0) {
            // the others: the block boundary nearest to each multiple of (what is in front of the last cut) / (n - 1)
            const double step = cand[last].second / (double)(n_target - 1);
            int prev_k = -1;
            for (int q = 1; q < n_target - 1; ++q) {
                int pick = -1;
                double bd = 1e9;
                for (int k = prev_k + 1; k < last; ++k) {
                    const double d = cand[k].second > q * step ? cand[k].second - q * step : q * step - cand[k].second;
                    if (d < bd) { bd = d; pick = k; }
                }
                if (pick < 0) break;
                cuts.push_back(cand[pick].first);
                prev_k = pick;
            }
            cuts.push_back(cand[last].first);
        }
    }
    cuts.push_back(0);
    if (cuts.size() <= 2) return;
    std::vector<PackItem> uitems;
    build_unpack_items(P, uitems);
    P->gb.resize(cuts.size() - 1);
    for (size_t b = 0; b + 1 < cuts.size(); ++b) {
        dmme_plan::GradBucket& G = P->gb[b];
        G.op_hi = cuts[b];
        G.op_lo = cuts[b + 1];
        const bool last = b + 2 == cuts.size();
        for (size_t pi = 0; pi < P->params.size(); ++pi) {
            const Param& pp = P->params[pi];  // (the sinusoid table, a buffer without gradient, rides in the last bucket: the
                                              // hand-overs then tile the whole flat buffer)
            const bool mine = owner[pi] < 0 ? last : (owner[pi] >= G.op_lo && owner[pi] < G.op_hi);
            if (!mine) continue;
            if (!G.ranges.empty() && G.ranges.back().first + G.ranges.back().second == pp.ref_off) G.ranges.back().second += pp.numel();
            else G.ranges.push_back({pp.ref_off, pp.numel()});
        }
        // (the tiled time-projection gradient addresses 64-column tiles: it exists only when every block's width is a multiple of
        // 64, and then so is every range start)
        for (size_t k = 0; k < P->tblocks.size(); ++k) {
            if (tcol_owner[k] < G.op_lo || tcol_owner[k] >= G.op_hi) continue;
            const int c0 = P->tblocks[k].col, c1 = c0 + P->tblocks[k].cout;
            if (!G.tcols.empty() && G.tcols.back().second == c0) G.tcols.back().second = c1;
            else G.tcols.push_back({c0, c1});
        }
        // unpack items follow the parameter order: a bucket's items are the runs inside its flat ranges
        for (int i = 0; i < (int)uitems.size(); ++i) {
            bool mine = false;
            for (auto& r : G.ranges) mine = mine || (uitems[i].src_off >= r.first && uitems[i].src_off < r.first + r.second);
            if (!mine) continue;
            if (!G.unpack.empty() && G.unpack.back().second == i) G.unpack.back().second = i + 1;
            else G.unpack.push_back({i, i + 1});
        }
    }
}

// Deferred reductions (one grouped launch each per backward or per bucket): the bias / time-projection rows of every conv, the
// per-image dbeta / dgamma rows of the GroupNorm in front of it, the column sums of dY; then every bucket's index range of each table.
static void plan_deferred_reductions(dmme_plan* P) {
    std::vector<int> bias_job_op, col_job_op;  // op index each job belongs to (gradient buckets)
    if (!debug_route("no_bias_group"))
        for (Op& o : P->ops) {
            if (o.kind != OP_CONV) continue;
            const int o_index = (int)(&o - P->ops.data());
            ConvArgs a{};
            fill_conv(P, o, nullptr, nullptr, nullptr, nullptr, nullptr, 1, a);
            if (o.gn >= 0 && o.b_gnrows >= 0) {
                // the norm in front of this conv: its backward leaves per-image dbeta / dgamma rows, summed over the batch by the same
                // grouped launch as the biases.  Bucket (gradient exchange overlap): by the NORM's op index, its jobs first.
                const Op& gop = P->ops[o.gn];
                const Tensor& t1 = P->tensors[gop.gn_src1];
                const int C = t1.C + (gop.gn_src2 >= 0 ? P->tensors[gop.gn_src2].C : 0);
                if (gn_route_of(P, o).rows) {
                    o.gn_rows_deferred = 1;
                    for (int which = 0; which < 2; ++which)
                        for (int cb = 0; cb < (C + 31) / 32; ++cb) {
                            BiasJob j{};
                            j.rowsum_off = o.b_gnrows + (int64_t)which * P->B * C * 4;
                            j.dbias_off = P->params[which == 0 ? gop.gn_beta : gop.gn_gamma].ref_off;
                            j.C = C;
                            j.cblock = cb;
                            j.tcol = -1;
                            P->bias_jobs.push_back(j);
                            bias_job_op.push_back(o.gn);
                        }
                }
            }
            if (!colsum_fast_supported(P->dtype, a.Hout * a.Wout, a.Cout)) continue;
            o.bias_deferred = 1;
            if (!debug_route("no_colsum_group")) {
                ColJob cj{};
                const int nch = colsum_group_chunks(P->dtype, a.Hout * a.Wout, a.Cout, &cj.chunk_px, &cj.ppw);
                cj.dy_off = o.dst == -2 ? P->bws_dy : P->gt_off[o.dst];
                cj.rowsum_off = o.b_rowsum;
                cj.HW = a.Hout * a.Wout;
                cj.C = a.Cout;
                for (int ch = 0; ch < nch; ++ch) {
                    cj.chunk = ch;
                    P->col_jobs.push_back(cj);
                    col_job_op.push_back(o_index);
                }
            }
            for (int cb = 0; cb < (a.Cout + 31) / 32; ++cb) {
                BiasJob j{};
                j.rowsum_off = o.b_rowsum;
                j.dbias_off = P->params[o.b].ref_off;
                j.C = a.Cout;
                j.cblock = cb;
                j.tcol = o.tproj_col;
                P->bias_jobs.push_back(j);
                bias_job_op.push_back(o_index);
            }
        }
    for (auto& G : P->gb) {  // jobs were pushed in ascending op order: a bucket's jobs are one index range
        auto range = [&](const std::vector<int>& ops_of, int& j0, int& j1) {
            j0 = j1 = 0;
            bool any = false, ok = true;
            for (int j = 0; j < (int)ops_of.size(); ++j) {
                if (ops_of[j] < G.op_lo || ops_of[j] >= G.op_hi) continue;
                if (!any) { j0 = j; any = true; } else if (j != j1) ok = false;
                j1 = j + 1;
            }
            return ok;
        };
        if (!range(bias_job_op, G.bias0, G.bias1) || !range(col_job_op, G.col0, G.col1)) {
            P->gb.clear();
            break;
        }
    }
}

// Batched time-projection gradients (dmme_plan::tp_tiles): where every block's width and column are multiples of 64.
static void plan_time_proj_tiles(dmme_plan* P) {
    bool ok = !P->tblocks.empty() && P->tproj_cols % 64 == 0;
    for (const auto& tb : P->tblocks) ok = ok && tb.cout % 64 == 0 && tb.col % 64 == 0;
    if (!ok) return;
    const int n64 = P->tproj_cols / 64;
    std::vector<int64_t> tiles(n64 + P->tproj_cols / 32, -1);
    for (const auto& tb : P->tblocks) {
        for (int r = 0; r < tb.cout; r += 64) tiles[(tb.col + r) / 64] = P->params[tb.tw].ref_off + (int64_t)r * P->cfg.emb_dim;
        for (int r = 0; r < tb.cout; r += 32) tiles[n64 + (tb.col + r) / 32] = P->params[tb.tb].ref_off + r;
    }
    for (int64_t v : tiles)
        if (v < 0) return;
    P->tp_tiles = tiles;
    P->tp_n64 = n64;
}

void plan_backward(dmme_plan* P) {
    layout_backward(P);
    plan_grad_buckets(P);
    for (auto& G : P->gb)  // before the "all" build: that one leaves the final Op::wg_layer values (and grows bws_bytes)
        for (int k = 0; k < 3; ++k) build_wgrad_group(P, G.wg[k], k, G.op_lo, G.op_hi);
    for (int k = 0; k < 3; ++k) build_wgrad_group(P, P->wg[k], k);
    plan_deferred_reductions(P);
    plan_time_proj_tiles(P);
}

}  // namespace dmme

extern "C" {

DMME_API int64_t dmme_unet_plan_packed_bwd_bytes(const dmme_plan* plan) { return plan ? plan->packed_bwd_bytes : 0; }
DMME_API int64_t dmme_unet_plan_bwd_workspace_bytes(const dmme_plan* plan) { return plan ? plan->bws_bytes : 0; }

DMME_API int dmme_unet_pack_params_bwd(const dmme_plan* plan, const float* ref_flat, void* packed_bwd, void* stream) {
    DMME_REQUIRE(plan && ref_flat && packed_bwd, DMME_ERR_INVALID, "pack_params_bwd: null argument");
    DMME_REQUIRE(plan->items_bwd_dev, DMME_ERR_INVALID, "pack_params_bwd: plan was created without a device");
    return launch_pack_table(plan->dtype, plan->items_bwd_dev.get(), plan->n_items_bwd, ref_flat, packed_bwd, (hipStream_t)stream);
}

// ---- the per-op routes of the reverse walk: each cascade written once.  The run-time facts enter as arguments: `weights` (false: the
// input-only form launches no parameter gradient of any kind), the grouped tables in force (a bucket's or the plan's), and - through
// the plan's device tables, which a host-only plan does not have - whether the grouped launches exist at all ----
enum AttnBwdRoute { ATTN_BWD_HEADS_MFMA, ATTN_BWD_HEADS, ATTN_BWD_MFMA, ATTN_BWD_GENERIC };
static AttnBwdRoute attn_bwd_route(const dmme_plan* P, const Op& o) {
    const Tensor& q = P->tensors[o.at_qkv];
    const int S = q.H * q.W, C = q.C / 3;
    if (o.at_heads > 1) return attn_heads_mfma_supported(P->dtype, P->B, S, C, o.at_heads) ? ATTN_BWD_HEADS_MFMA : ATTN_BWD_HEADS;
    return attn_bwd_mfma_supported(P->dtype, P->B, S, C) ? ATTN_BWD_MFMA : ATTN_BWD_GENERIC;
}

// bias and time-embedding-row gradients (column sums of dY).  GROUPED: column sums and reduction both come from the grouped launches of
// the flush; FAST_COLSUMS: column sums now, reduction in the grouped launch; FAST / GENERIC: both now
enum BiasRoute { BIAS_NONE, BIAS_GROUPED, BIAS_FAST_COLSUMS, BIAS_FAST, BIAS_GENERIC };
static BiasRoute bias_route(const dmme_plan* P, const Op& o, const ConvArgs& a, bool weights) {
    if (!weights) return BIAS_NONE;
    if (o.bias_deferred && P->bias_jobs_dev) return P->col_jobs_dev ? BIAS_GROUPED : BIAS_FAST_COLSUMS;
    return colsum_fast_supported(P->dtype, a.Hout * a.Wout, a.Cout) ? BIAS_FAST : BIAS_GENERIC;
}

// weight gradient.  GROUPED: deferred to the grouped launch of the flush (wg: the tables in force); else per layer, into the packed
// image (MFMA) or the reference layout
enum WgradRoute { WGRAD_NONE, WGRAD_GROUPED, WGRAD_MFMA, WGRAD_SMALL, WGRAD_GENERIC };
static WgradRoute wgrad_route(const dmme_plan* P, const Op& o, const ConvArgs& a, bool weights, const dmme_plan::WgGroup* wg) {
    if (!weights) return WGRAD_NONE;
    if (o.wg_layer >= 0 && wg[wg_index(o)].jobs_dev) return WGRAD_GROUPED;
    if (wgrad_mfma_supported(P->dtype, a)) return WGRAD_MFMA;
    return wgrad_small_supported(P->dtype, a) ? WGRAD_SMALL : WGRAD_GENERIC;
}

// The data gradient of conv o (forward arguments a): the forward kernels on dY with transposed, tap-flipped weights w.  splitk: the
// forward workspace's split-K scratch (null: none offered)
static ConvArgs dgrad_args(const dmme_plan* P, const Op& o, const ConvArgs& a, const void* dy, const void* w, void* dst, float* splitk) {
    ConvArgs d{};
    d.src1 = dy; d.w = w; d.dst = dst;
    d.N = P->B; d.C1 = a.Cout; d.Hin = a.Hout; d.Win = a.Wout; d.Cout = a.C1 + a.C2;
    d.up = o.stride == 2 ? 2 : 0;
    d.stride = 1; d.taps = o.taps;
    d.Hout = d.up ? 2 * d.Hin : d.Hin;
    d.Wout = d.up ? 2 * d.Win : d.Win;
    d.x3 = P->x3;
    d.f16 = P->dtype == DMME_F16;  // (launchers without a dtype argument: conv1x1_as, the thin output conv)
    if (splitk && P->splitk_floats > 0) {
        d.splitk = splitk;
        d.splitk_cap = P->splitk_floats;
    }
    return d;
}

// One backward pass: the state of the reverse walk and its steps, in the order backward_impl calls them.
struct BwdRun {
    const dmme_plan* P;
    const char *pk, *pkb;  // packed weights: forward layout, data-gradient layout
    const float *x, *d_y;  // network input; d_y: NCHW fp32, or the classifier's d logits
    char *ws, *bws;
    const float* drop_masks;
    float *grad_flat, *d_x;  // grad_flat == nullptr: the input-only backward - d_x alone, no weight-gradient launch of any kind
    hipStream_t s;
    dmme_bucket_fn ready;
    void* user;
    const int B, dt, nt, G;
    const bool weights;
    const bool buckets;  // bucketed mode: deferred work flushed per gradient bucket
    const bool res_extra_off, dgrad_direct_off, time_pre_off;  // (switches: one read per backward)
    std::vector<char> written;         // per tensor: its gradient buffer holds a contribution
    // identity-residual branches (d x += d out of a ResBlock / attention block) are not launched on their own: the pointer waits here
    // until the GroupNorm backward that writes x's gradient anyway (norm1 / the attention norm of the same block) takes it as one more
    // addend; anything else that needs x's gradient first gets it through flush_pending
    std::vector<const char*> pending;
    int next_bucket = 0;  // the bucket whose stretch the reverse walk is in
    float *wimage, *dtproj, *sink;  // sink: input-only form, the GroupNorm backward's d gamma / d beta land here, unread
    char* tmp;
    const int64_t* labels = nullptr;  // conditional plans: the labels of the forward this backward follows

    BwdRun(const dmme_plan* plan, const void* packed, const void* packed_bwd, const float* x_, int t_len, const float* dy_, void* workspace, void* bwd_workspace,
           const float* masks, float* grad, float* dx, void* stream, dmme_bucket_fn ready_, void* user_)
        : P(plan), pk((const char*)packed), pkb((const char*)packed_bwd), x(x_), d_y(dy_), ws((char*)workspace), bws((char*)bwd_workspace), drop_masks(masks),
          grad_flat(grad), d_x(dx), s((hipStream_t)stream), ready(ready_), user(user_), B(plan->B), dt(plan->dtype), nt(t_len), G(plan->cfg.num_groups),
          weights(grad != nullptr), buckets(grad != nullptr && ready_ != nullptr && !plan->gb.empty()), res_extra_off(debug_route("no_res_extra") != 0),
          dgrad_direct_off(debug_route("no_dgrad_direct") != 0), time_pre_off(debug_route("no_time_pre") != 0), written(plan->tensors.size(), 0),
          pending(plan->tensors.size(), nullptr), wimage((float*)(bws + plan->bws_wimage)), dtproj((float*)(bws + plan->bws_dtproj)),
          sink((float*)(bws + plan->bws_sink)), tmp(bws + plan->bws_tmp) {}

    char* gptr(int id) const { return bws + P->gt_off[id]; }
    const char* dy_of(const Op& o) const { return o.dst == -2 ? bws + P->bws_dy : gptr(o.dst); }
    int claim(int id) {  // 0: first contribution (write), 1: accumulate
        const int acc = written[id];
        written[id] = 1;
        return acc;
    }
    float* pgrad(int param, int which) const { return weights ? grad_flat + P->params[param].ref_off : sink + which * P->sink_half; }
    int flush_pending(int id) {
        if (id < 0 || !pending[id]) return DMME_OK;
        const Tensor& t = P->tensors[id];
        const char* src = pending[id];
        pending[id] = nullptr;
        const int acc = claim(id);
        return launch_grad_acc(dt, src, gptr(id), nullptr, t.C, 0, acc, 0, 0, B, t.H, t.W, s);
    }
    void hand_over(int b) const {
        for (const auto& r : P->gb[b].ranges) ready(user, b, r.first, r.second);
    }
    // has the walk, about to run op oi, left the stretch of the bucket it is in?
    bool bucket_done(int oi) const { return buckets && next_bucket + 1 < (int)P->gb.size() && oi == P->gb[next_bucket].op_lo - 1; }
    // every op of this bucket has run (a pending identity-residual gradient that belongs to a tensor of the NEXT stretch stays pending:
    // it carries no parameter gradient): finish the bucket's parameter gradients and hand it to the exchange
    int finish_bucket() {
        const int rc = flush(next_bucket);
        if (rc != DMME_OK) return rc;
        hand_over(next_bucket);
        ++next_bucket;
        return DMME_OK;
    }

    // clears the accumulators, brings d_y into the walk's layout; the classifier's head
    int head() {
        // (the region holds only accumulators of weight gradients and column sums: the input-only form reads none of it)
        if (weights) DMME_CHECK_HIP(hipMemsetAsync(bws + P->bws_zero, 0, (size_t)P->bws_zero_bytes, s));
        // (the first launch: it checks the device-side mark of the forward form, which a replayed no-grad graph sets without the host seeing it)
        // classifier: d_y is d logits (B, K) fp32 - copied as is (HW = 1, fp32) through the same mark check
        const bool cls = P->head_src >= 0;
        int rc = launch_nchw_to_nhwc(cls ? DMME_F32 : dt, d_y, B, P->out_channels, cls ? 1 : P->H * P->W, bws + P->bws_dy, s, (const unsigned*)(ws + P->ws_mark),
                                     P->err_host.get());
        if (rc != DMME_OK) return rc;
        if (cls) {  // the head: d logits -> d(top map), written whole; its parameters' gradients (weights form only)
            const Tensor& tt = P->tensors[P->head_src];
            const float* dlog = (const float*)(bws + P->bws_dy);
            float* pool = weights ? (float*)(bws + P->bws_hpool) : nullptr;
            float* hrows = weights ? (float*)(bws + P->bws_hrows) : nullptr;
            rc = launch_cls_head_bwd(dt, ws + tt.off, B, tt.H * tt.W, tt.C, G, (const float*)(pk + P->params[P->p_hgw].packed_off),
                                     (const float*)(pk + P->params[P->p_hgb].packed_off), (const float*)(pk + P->params[P->p_hw].packed_off), P->out_channels, dlog,
                                     gptr(P->head_src), pool, hrows, s);
            if (rc == DMME_OK && weights)
                rc = launch_cls_head_wgrad(dlog, pool, hrows, B, P->out_channels, tt.C, grad_flat + P->params[P->p_hw].ref_off, grad_flat + P->params[P->p_hb].ref_off,
                                           grad_flat + P->params[P->p_hgw].ref_off, grad_flat + P->params[P->p_hgb].ref_off, s);
            if (rc != DMME_OK) return rc;
            written[P->head_src] = 1;
        }
        if (weights && P->cfg.arch == DMME_ARCH_IDDPM && nt == 1)  // shared timestep row: the GroupNorm backward accumulates into it atomically
            DMME_CHECK_HIP(hipMemsetAsync(dtproj, 0, (size_t)P->tproj_cols * 4, s));
        return DMME_OK;
    }

    int attention(const Op& o) {
        int rc = flush_pending(o.at_out);
        if (rc != DMME_OK) return rc;
        const Tensor& q = P->tensors[o.at_qkv];
        const int S = q.H * q.W, C = q.C / 3;
        DMME_REQUIRE(written[o.at_out], DMME_ERR_INVALID, "backward: attention output has no gradient");
        switch (attn_bwd_route(P, o)) {
            case ATTN_BWD_HEADS_MFMA:
                rc = launch_attn_heads_bwd_mfma(dt, ws + q.off, ws + P->tensors[o.at_out].off, gptr(o.at_out), (const float*)(ws + o.at_lse), B, S, C,
                                                o.at_heads, bws + P->bws_attP, bws + P->bws_attdS, gptr(o.at_qkv), s);
                break;
            case ATTN_BWD_HEADS:
                rc = launch_attn_heads_bwd(dt, ws + q.off, gptr(o.at_out), B, S, C, o.at_heads, (float*)(bws + P->bws_attP),
                                           (float*)(bws + P->bws_attdS), gptr(o.at_qkv), s);
                break;
            case ATTN_BWD_MFMA:
                rc = launch_attn_bwd_mfma(dt, ws + q.off, ws + P->tensors[o.at_out].off, gptr(o.at_out), (const float*)(ws + o.at_lse), B, S, C,
                                          bws + P->bws_attP, bws + P->bws_attdS, gptr(o.at_qkv), s);
                break;
            default:
                rc = launch_attn_bwd_generic(dt, ws + q.off, gptr(o.at_out), B, S, C, (float*)(bws + P->bws_attP),
                                             (float*)(bws + P->bws_attdS), gptr(o.at_qkv), s);
        }
        written[o.at_qkv] = 1;
        return rc;
    }

    // the gradient of the conv's output is complete before anything reads it
    int conv_dy(const Op& o) {
        if (o.dst >= 0) {
            const int rc = flush_pending(o.dst);
            if (rc != DMME_OK) return rc;
        }
        if (o.dst != -2) DMME_REQUIRE(written[o.dst], DMME_ERR_INVALID, "backward: tensor %d has no gradient", o.dst);
        return DMME_OK;
    }
    // 1. bias and time-embedding-row gradients (column sums of dY)
    int conv_bias(const Op& o, const ConvArgs& a) {
        const char* dy = dy_of(o);
        float* rowsum = (float*)(bws + o.b_rowsum);
        switch (bias_route(P, o, a, weights)) {
            case BIAS_FAST_COLSUMS:
                return launch_colsum_fast(dt, dy, B, a.Hout * a.Wout, a.Cout, rowsum, nullptr, nullptr, P->tproj_cols, nt, s);
            case BIAS_FAST:
                return launch_colsum_fast(dt, dy, B, a.Hout * a.Wout, a.Cout, rowsum, grad_flat + P->params[o.b].ref_off,
                                          o.tproj_col >= 0 ? dtproj + o.tproj_col : nullptr, P->tproj_cols, nt, s);
            case BIAS_GENERIC:
                return launch_colsum(dt, dy, B, a.Hout * a.Wout, a.Cout, rowsum, grad_flat + P->params[o.b].ref_off,
                                     o.tproj_col >= 0 ? dtproj + o.tproj_col : nullptr, P->tproj_cols, nt, s);
            default: return DMME_OK;  // (input-only form; or its column sums come from the grouped launch of the flush)
        }
    }
    // 2. weight gradient: deferred to the grouped launch of the flush, or per layer (packed image / reference layout)
    int conv_wgrad(const Op& o, const ConvArgs& a) {
        const char* dy = dy_of(o);
        switch (wgrad_route(P, o, a, weights, buckets ? P->gb[next_bucket].wg : P->wg)) {
            case WGRAD_MFMA: return launch_wgrad_mfma(dt, a, dy, wimage + P->params[o.w].wp_off, s);
            case WGRAD_SMALL: return launch_wgrad_small(dt, a, dy, grad_flat + P->params[o.w].ref_off, s);
            case WGRAD_GENERIC: return launch_wgrad_generic(dt, a, dy, grad_flat + P->params[o.w].ref_off, s);
            default: return DMME_OK;  // (input-only form; or grouped)
        }
    }
    // 3. data gradient into the source's gradient buffer(s), through the backward of the norm in front of the conv where there is one
    int conv_dgrad(const Op& o, const ConvArgs& a) {
        ConvArgs d = dgrad_args(P, o, a, dy_of(o), pkb + P->params[o.w].packed_bwd_off, tmp, (float*)(ws + P->ws_splitk));
        const Tensor& t1 = P->tensors[o.src1];
        const int Cin = a.C1 + a.C2;
        const GnBwdRoute gr = o.gn >= 0 ? gn_route_of(P, o) : GnBwdRoute{};
        char* g1 = gptr(o.src1);
        char* g2 = o.src2 >= 0 ? gptr(o.src2) : nullptr;
        const char* extra = nullptr;  // a waiting residual branch of the source: taken along by the GroupNorm backward below
        int rc = DMME_OK;
        if (pending[o.src1]) {
            if (o.gn >= 0 && o.src2 < 0 && gr.takes_extra) {
                extra = pending[o.src1];
                pending[o.src1] = nullptr;
            } else {
                rc = flush_pending(o.src1);
                if (rc != DMME_OK) return rc;
            }
        }
        if (o.src2 >= 0) {
            rc = flush_pending(o.src2);
            if (rc != DMME_OK) return rc;
        }
        const int acc1 = claim(o.src1), acc2 = o.src2 >= 0 ? claim(o.src2) : 0;
        // a conv with no norm in front of it, one source and no fused upsample: its data gradient IS the source's gradient -
        // written (or, through the epilogue's residual input, accumulated in place: each vector is read and written by one thread)
        // straight into that buffer instead of a scratch tensor plus an accumulation launch
        const bool dgrad_direct = !dgrad_direct_off && o.gn < 0 && o.src2 < 0 && o.up != 1;
        if (dgrad_direct) {
            d.dst = g1;
            if (acc1) {
                d.res1 = g1;
                d.R1 = Cin;
            }
        }
        rc = launch_conv(dt, d, s);
        if (rc != DMME_OK) return rc;
        if (o.gn < 0) return dgrad_direct ? DMME_OK : launch_grad_acc(dt, tmp, g1, g2, a.C1, a.C2, acc1, acc2, o.up == 1 ? 1 : 0, B, t1.H, t1.W, s);
        const Op& gop = P->ops[o.gn];
        GnMod mod{};
        if (gop.gn_mod_col >= 0) {  // scale-shift conditioning: effective gamma + gradients of the (shift | scale) projection rows
            mod.t_scale = (const float*)(ws + P->ws_tproj) + gop.gn_mod_col + gop.gn_mod_C;
            mod.beta = (const float*)(pk + P->params[gop.gn_beta].packed_off);
            mod.d_shift = dtproj + gop.gn_mod_col;
            mod.d_scale = dtproj + gop.gn_mod_col + gop.gn_mod_C;
            mod.ld = P->tproj_cols;
            mod.nt = nt;
        }
        return launch_gn_bwd(gr, dt, tmp, a.src1, a.src2, B, t1.H * t1.W, a.C1, a.C2, G, (const float*)(pk + P->params[gop.gn_gamma].packed_off),
                             (const float*)(ws + gop.gn_mr), a.scale, a.shift, a.dmask, a.pro_silu, g1, g2, acc1, acc2, pgrad(gop.gn_gamma, 0),
                             pgrad(gop.gn_beta, 1), (float*)(bws + o.b_ab), (float*)(bws + P->bws_gnS), mod, s,
                             weights && o.wg_act >= 0 ? bws + o.wg_act : nullptr,
                             weights && o.gn_rows_deferred && P->bias_jobs_dev ? (float*)(bws + o.b_gnrows) : nullptr, extra);
    }
    // gradient with respect to the network input (NCHW fp32), only on request
    int input_grad(const Op& o, const ConvArgs& a) {
        ConvArgs d = dgrad_args(P, o, a, dy_of(o), pkb + P->params[o.w].packed_bwd_off, d_x, nullptr);
        d.out_nchw = 1;
        return launch_conv(dt, d, s, 2);  // (the first-generation MFMA kernel where it applies, else the generic one)
    }
    // 4. residual branch: d(res) += dY
    int residual(const Op& o, const ConvArgs& a) {
        if (o.res1 < 0) return DMME_OK;
        if (o.res_alias) {
            written[o.res1] = 1;  // (its gradient buffer is dY itself)
            return DMME_OK;
        }
        const char* dy = dy_of(o);
        const int R1 = P->tensors[o.res1].C;
        if (!res_extra_off && o.res2 < 0 && R1 == a.Cout && o.dst >= 0) {
            const int rc = flush_pending(o.res1);  // (one waiting branch per tensor)
            pending[o.res1] = dy;
            return rc;
        }
        const int acc1 = claim(o.res1), acc2 = o.res2 >= 0 ? claim(o.res2) : 0;
        return launch_grad_acc(dt, dy, gptr(o.res1), o.res2 >= 0 ? gptr(o.res2) : nullptr, R1, a.Cout - R1, acc1, acc2, 0, B, a.Hout, a.Wout, s);
    }

    // deferred launches of one gradient bucket (b >= 0) or of everything (b = -1): bias + time rows, grouped weight gradients, unpack,
    // the per-block time-projection weight gradients
    int flush(int b) {
        int r = DMME_OK;
        const int emb = P->cfg.emb_dim, tc = P->tproj_cols;
        const float* temb = (const float*)(ws + P->ws_temb);
        const dmme_plan::GradBucket* GBk = b >= 0 ? &P->gb[b] : nullptr;
        if (P->bias_jobs_dev && P->col_jobs_dev) {
            const int j0 = GBk ? GBk->col0 : 0, j1 = GBk ? GBk->col1 : (int)P->col_jobs.size();
            if (j1 > j0) r = launch_colsum_group(dt, P->col_jobs_dev.get() + j0, j1 - j0, bws, B, s);
            if (r != DMME_OK) return r;
        }
        if (P->bias_jobs_dev) {
            const int j0 = GBk ? GBk->bias0 : 0, j1 = GBk ? GBk->bias1 : (int)P->bias_jobs.size();
            if (j1 > j0) r = launch_bias_tproj_group(P->bias_jobs_dev.get() + j0, j1 - j0, bws, grad_flat, dtproj, B, tc, nt, s);
            if (r != DMME_OK) return r;
        }
        for (int k = 0; k < 3; ++k) {
            const dmme_plan::WgGroup& G = GBk ? GBk->wg[k] : P->wg[k];
            if (!G.jobs_dev) continue;
            r = launch_wgrad_group(dt, G.taps, G.layers_dev.get(), G.jobs_dev.get(), (int)G.jobs.size(), ws, bws, drop_masks, wimage, s, G.dma, bws + P->bws_zpage);
            if (r != DMME_OK) return r;
        }
        {
            std::vector<std::pair<int, int>> all_items{{0, P->n_items_unpack}};
            for (const auto& ir : (GBk ? GBk->unpack : all_items)) {
                if (ir.second > ir.first) r = launch_wgrad_unpack(P->items_unpack_dev.get() + ir.first, ir.second - ir.first, wimage, grad_flat, s);
                if (r != DMME_OK) return r;
            }
        }
        std::vector<std::pair<int, int>> all_cols{{0, tc}};
        for (const auto& cr : (GBk ? GBk->tcols : all_cols)) {
            const int c0 = cr.first, c1 = cr.second;
            if (c1 <= c0) continue;
            if (P->tp_tiles_dev) {  // every block's dW / db in one launch each
                r = launch_small_gemm_tn_tiled(dtproj + c0, tc, temb, emb, c1 - c0, emb, nt, grad_flat, emb, P->tp_tiles_dev.get() + c0 / 64, s);
                if (r == DMME_OK) r = launch_nsum_tiled(dtproj + c0, nt, c1 - c0, tc, 1, grad_flat, P->tp_tiles_dev.get() + P->tp_n64 + c0 / 32, s);
                if (r != DMME_OK) return r;
            } else {
                for (const auto& tb : P->tblocks) {
                    if (tb.col < c0 || tb.col >= c1) continue;
                    // dW_block[o][k] += sum_r dtproj[r][col+o] temb[r][k];  db_block[o] += sum_r dtproj[r][col+o]
                    r = launch_small_gemm(dt, 2, dtproj + tb.col, tc, temb, emb, tb.cout, emb, nt, nullptr, 0, grad_flat + P->params[tb.tw].ref_off, emb, s);
                    if (r == DMME_OK) r = launch_nsum(dtproj + tb.col, nt, tb.cout, tc, 1, grad_flat + P->params[tb.tb].ref_off, s);
                    if (r != DMME_OK) return r;
                }
            }
        }
        return r;
    }

    // time MLP backward (models/ddpm.py:211-217 and the per-block Linear at :101-104); hands over the last bucket
    int time_mlp() {
        const int emb = P->cfg.emb_dim, pos = P->cfg.pos_dim, tc = P->tproj_cols;
        const float* h1 = (const float*)(ws + P->ws_th1);
        const float* esin = (const float*)(ws + P->ws_tsin);
        float* dtemb = (float*)(bws + P->bws_dtemb);
        float* dh1 = (float*)(bws + P->bws_dh1);
        float* z = (float*)(bws + P->bws_z);
        // input gradients of the Linears as NT GEMMs against a transposed copy of the weights (K contiguous in both operands)
        char* wT = bws + P->bws_wT;
        int rc = launch_transpose(dt, pk + P->tproj_w_off, tc, emb, wT, s);
        if (rc == DMME_OK) rc = launch_small_gemm(dt, 0, dtproj, tc, wT, tc, nt, emb, tc, nullptr, 0, dtemb, emb, s);
        if (rc != DMME_OK) return rc;
        // temb = silu(z2), z2 = h1 W2^T + b2
        // (the forward kept both pre-activations when it ran at a training batch: no recompute GEMMs here)
        const bool saved_pre = nt > 4 && P->ws_tz1 >= 0 && P->ws_tz2 >= 0 && !time_pre_off;
        if (saved_pre || P->cond)  // (a conditional forward always keeps z2 + E[y] there: the label op wrote it)
            z = (float*)(ws + P->ws_tz2);
        else
            rc = launch_small_gemm(dt, 0, h1, emb, pk + P->params[P->p_l2w].packed_off, emb, nt, emb, emb, (const float*)(pk + P->params[P->p_l2b].packed_off), 0, z, emb, s);
        if (rc == DMME_OK) rc = launch_silu_bwd(dtemb, z, nt * emb, s);
        if (rc == DMME_OK && P->cond)  // dtemb holds d z2 now: the label rows take their images' sums
            rc = launch_label_grad(dtemb, labels, B, P->cfg.num_classes, emb, grad_flat + P->params[P->p_lemb].ref_off, s);
        if (rc == DMME_OK) rc = launch_small_gemm(dt, 2, dtemb, emb, h1, emb, emb, emb, nt, nullptr, 0, grad_flat + P->params[P->p_l2w].ref_off, emb, s);
        if (rc == DMME_OK) rc = launch_nsum(dtemb, nt, emb, emb, 1, grad_flat + P->params[P->p_l2b].ref_off, s);
        if (rc == DMME_OK) rc = launch_transpose(dt, pk + P->params[P->p_l2w].packed_off, emb, emb, wT, s);
        if (rc == DMME_OK) rc = launch_small_gemm(dt, 0, dtemb, emb, wT, emb, nt, emb, emb, nullptr, 0, dh1, emb, s);
        // h1 = silu(z1), z1 = e W1^T + b1
        if (saved_pre)
            z = (float*)(ws + P->ws_tz1);
        else if (rc == DMME_OK)
            rc = launch_small_gemm(dt, 0, esin, pos, pk + P->params[P->p_l1w].packed_off, pos, nt, emb, pos, (const float*)(pk + P->params[P->p_l1b].packed_off), 0, z, emb, s);
        if (rc == DMME_OK) rc = launch_silu_bwd(dh1, z, nt * emb, s);
        if (rc == DMME_OK) rc = launch_small_gemm(dt, 2, dh1, emb, esin, pos, emb, pos, nt, nullptr, 0, grad_flat + P->params[P->p_l1w].ref_off, pos, s);
        if (rc == DMME_OK) rc = launch_nsum(dh1, nt, emb, emb, 1, grad_flat + P->params[P->p_l1b].ref_off, s);
        if (rc == DMME_OK && buckets) hand_over((int)P->gb.size() - 1);
        return rc;
    }
};

static int backward_impl(const dmme_plan* plan, const void* packed, const void* packed_bwd, const float* x, const int64_t* t, int t_len,
                         const float* d_y, void* workspace, void* bwd_workspace, const float* drop_masks, float* grad_flat, float* d_x,
                         void* stream, dmme_bucket_fn ready, void* user, const int64_t* labels = nullptr) {
    const bool weights = grad_flat != nullptr;  // (false: dmme_unet_backward_input)
    DMME_REQUIRE(plan && packed && packed_bwd && x && t && d_y && workspace && bwd_workspace && (weights || d_x), DMME_ERR_INVALID,
                 "unet_backward: null argument");
    DMME_REQUIRE(t_len == 1 || t_len == plan->B, DMME_ERR_INVALID, "unet_backward: bad t_len %d", t_len);
    DMME_REQUIRE((plan->cond != 0) == (labels != nullptr), DMME_ERR_INVALID,
                 plan->cond ? "unet_backward: a class-conditional plan (DMME_ARCH_DDPM_COND) takes labels: call dmme_unet_backward_cond / dmme_unet_backward_input_cond"
                            : "unet_backward_cond: the plan is not class-conditional (DMME_ARCH_DDPM_COND)");
    // (the conditional forward ran with one time row per image behind the label op: a shared t has no per-row gradient to reduce)
    DMME_REQUIRE(!plan->cond || !weights || t_len == plan->B, DMME_ERR_INVALID,
                 "unet_backward_cond: parameter gradients need one timestep per image (t_len = %d, B = %d)", t_len, plan->B);
    if (plan->cond) t_len = plan->B;  // what the forward's ops behind the label op ran with
    if (int rc0 = lvl_check(plan, "unet_backward", (hipStream_t)stream, true)) return rc0;  // (the forward this backward differentiates ran through the engine)
    DMME_REQUIRE(!plan->mix, DMME_ERR_UNSUPPORTED, "unet_backward: precision fp16r32 is an inference mode");
    DMME_REQUIRE(plan->nograd_ws != workspace, DMME_ERR_INVALID,
                 "unet_backward: the last forward into this workspace was dmme_unet_forward_nograd / dmme_chain_step, which leave out the tensors only a "
                 "backward pass reads; run dmme_unet_forward first");
    const dmme_plan* P = plan;
    BwdRun R(P, packed, packed_bwd, x, t_len, d_y, workspace, bwd_workspace, drop_masks, grad_flat, d_x, stream, ready, user);
    R.labels = labels;
    int rc = R.head();
    for (int oi = (int)P->ops.size() - 1; oi >= 0 && rc == DMME_OK; --oi) {
        if (R.bucket_done(oi)) {
            rc = R.finish_bucket();
            if (rc != DMME_OK) break;
        }
        const Op& o = P->ops[oi];
        if (o.kind == OP_ATTN) rc = R.attention(o);
        if (o.kind != OP_CONV) continue;
        ConvArgs a{};
        fill_conv(P, o, R.pk, x, nullptr, R.ws, drop_masks, t_len, a);
        rc = R.conv_dy(o);
        if (rc == DMME_OK) rc = R.conv_bias(o, a);
        if (rc == DMME_OK) rc = R.conv_wgrad(o, a);
        if (rc == DMME_OK && o.src1 >= 0) rc = R.conv_dgrad(o, a);
        if (rc == DMME_OK && o.src1 == -2 && d_x) rc = R.input_grad(o, a);
        if (rc == DMME_OK) rc = R.residual(o, a);
    }
    for (int id = 0; id < (int)R.pending.size() && rc == DMME_OK; ++id) rc = R.flush_pending(id);
    if (rc != DMME_OK || !weights) return rc;
    rc = R.flush(R.buckets ? (int)P->gb.size() - 1 : -1);
    if (rc != DMME_OK) return rc;
    return R.time_mlp();
}

DMME_API int dmme_unet_backward(const dmme_plan* plan, const void* packed, const void* packed_bwd, const float* x,
                                const int64_t* t, int t_len, const float* d_y, void* workspace, void* bwd_workspace,
                                const float* drop_masks, float* grad_flat, float* d_x, void* stream) {
    DMME_REQUIRE(grad_flat, DMME_ERR_INVALID, "unet_backward: null argument (grad_flat)");
    return backward_impl(plan, packed, packed_bwd, x, t, t_len, d_y, workspace, bwd_workspace, drop_masks, grad_flat, d_x, stream, nullptr, nullptr);
}

DMME_API int dmme_unet_backward_input(const dmme_plan* plan, const void* packed, const void* packed_bwd, const float* x, const int64_t* t,
                                      int t_len, const float* d_y, void* workspace, void* bwd_workspace, const float* drop_masks, float* d_x,
                                      void* stream) {
    DMME_REQUIRE(d_x, DMME_ERR_INVALID, "unet_backward_input: d_x is required");
    return backward_impl(plan, packed, packed_bwd, x, t, t_len, d_y, workspace, bwd_workspace, drop_masks, nullptr, d_x, stream, nullptr, nullptr);
}

DMME_API int dmme_unet_backward_buckets(const dmme_plan* plan, const void* packed, const void* packed_bwd, const float* x,
                                        const int64_t* t, int t_len, const float* d_y, void* workspace, void* bwd_workspace,
                                        const float* drop_masks, float* grad_flat, float* d_x, void* stream, dmme_bucket_fn ready, void* user) {
    DMME_REQUIRE(grad_flat, DMME_ERR_INVALID, "unet_backward: null argument (grad_flat)");
    DMME_REQUIRE(ready, DMME_ERR_INVALID, "unet_backward_buckets: null callback");
    return backward_impl(plan, packed, packed_bwd, x, t, t_len, d_y, workspace, bwd_workspace, drop_masks, grad_flat, d_x, stream, ready, user);
}

DMME_API int dmme_unet_backward_cond(const dmme_plan* plan, const void* packed, const void* packed_bwd, const float* x, const int64_t* t, int t_len,
                                     const int64_t* labels, const float* d_y, void* workspace, void* bwd_workspace, const float* drop_masks,
                                     float* grad_flat, float* d_x, void* stream, dmme_bucket_fn ready, void* user) {
    DMME_REQUIRE(grad_flat && labels, DMME_ERR_INVALID, "unet_backward_cond: null argument (grad_flat / labels)");
    return backward_impl(plan, packed, packed_bwd, x, t, t_len, d_y, workspace, bwd_workspace, drop_masks, grad_flat, d_x, stream, ready, user, labels);
}

DMME_API int dmme_unet_backward_input_cond(const dmme_plan* plan, const void* packed, const void* packed_bwd, const float* x, const int64_t* t,
                                           int t_len, const int64_t* labels, const float* d_y, void* workspace, void* bwd_workspace,
                                           const float* drop_masks, float* d_x, void* stream) {
    DMME_REQUIRE(d_x && labels, DMME_ERR_INVALID, "unet_backward_input_cond: d_x and labels are required");
    return backward_impl(plan, packed, packed_bwd, x, t, t_len, d_y, workspace, bwd_workspace, drop_masks, nullptr, d_x, stream, nullptr, nullptr, labels);
}

DMME_API int dmme_unet_plan_grad_buckets(const dmme_plan* plan, int64_t* offsets, int64_t* numels, int* bucket_of, int cap) {
    DMME_REQUIRE(plan && offsets && numels && cap > 0, DMME_ERR_INVALID, "grad_buckets: bad argument");
    if (plan->gb.empty()) {  // no clean cut for this configuration: one piece
        offsets[0] = 0;
        numels[0] = plan->ref_numel;
        if (bucket_of) bucket_of[0] = 0;
        return 1;
    }
    int n = 0;
    for (size_t b = 0; b < plan->gb.size(); ++b)
        for (const auto& r : plan->gb[b].ranges) {
            if (n < cap) {
                offsets[n] = r.first;
                numels[n] = r.second;
                if (bucket_of) bucket_of[n] = (int)b;
            }
            ++n;
        }
    return n;
}

/* Which kernels a backward of this plan launches, as "key=value" pairs: the grouped weight-gradient layers / jobs per kernel
 * size, the grouped column-sum and bias jobs, and how many DATA-gradient convolutions run on each forward kernel (by label).
 * Lets a parity test assert that a configuration really exercises the kernels it is meant to cover. */
DMME_API int dmme_unet_plan_bwd_summary(const dmme_plan* plan, char* buf, int cap) {
    DMME_REQUIRE(plan && buf && cap > 0, DMME_ERR_INVALID, "bwd_summary: bad argument");
    const dmme_plan* P = plan;
    std::string out;
    char tmp[256];
    snprintf(tmp, sizeof(tmp), "wgrad_group3x3_layers=%d wgrad_group3x3_jobs=%d wgrad_group1x1_layers=%d wgrad_group1x1_jobs=%d colsum_group_jobs=%d bias_group_jobs=%d",
             (int)P->wg[0].layers.size(), (int)P->wg[0].jobs.size(), (int)P->wg[1].layers.size(), (int)P->wg[1].jobs.size(), (int)P->col_jobs.size(),
             (int)P->bias_jobs.size());
    out = tmp;
    std::unordered_map<std::string, int> dgrad;
    for (const Op& o : P->ops) {
        if (o.kind != OP_CONV || o.src1 < 0) continue;
        ConvArgs a{};
        fill_conv(P, o, (const char*)4096, (const float*)4096, (float*)4096, (char*)4096, nullptr, 1, a);
        const ConvArgs d = dgrad_args(P, o, a, (const void*)4096, (const void*)4096, (void*)4096, (float*)4096);
        char label[128] = "generic";
        const ConvRoute r = conv_route(P->dtype, d);
        if (r.family != CONV_GENERIC) conv_label(r, P->dtype, d, label, sizeof(label));
        dgrad[label] += 1;
    }
    for (const auto& kv : dgrad) {
        snprintf(tmp, sizeof(tmp), " dgrad[%s]=%d", kv.first.c_str(), kv.second);
        out += tmp;
    }
    strncpy(buf, out.c_str(), (size_t)cap - 1);
    buf[cap - 1] = 0;
    return DMME_OK;
}

}  // extern "C"
