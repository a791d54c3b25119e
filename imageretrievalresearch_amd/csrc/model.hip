// Model object behind the C ABI: tensor table, one-time weight pack (BN fold -> bf16 -> kernel layout),
// arena, and the executor that walks the op plan launching the HIP kernels on the caller's stream.
// Replaces timm.create_model(...) + .forward/.forward_features (see include/mi355_retrieval.h).
#include "model_exec.h"
#include "../../include/mi355_retrieval.h"

#include <string.h>

#include <algorithm>

namespace mi355 {

int pack_gemm(Packer& pk, Op& op) {
    const TensorSpec* w = pk.get(op.w_name);
    if (!w) return ERR_STATE;
    const int N = op.cout_real, K = op.cin_real;
    MI355_REQUIRE(w->numel() == (int64_t)N * K, "pack: %s has %lld elements, expected %d x %d", op.w_name.c_str(),
                  (long long)w->numel(), N, K);
    std::vector<float> scale, shift;
    if (!pk.bn_fold(op.bn_name, op.bn_eps, N, scale, shift)) return ERR_STATE;
    if (!op.bias_name.empty()) {
        const TensorSpec* b = pk.get(op.bias_name);
        if (!b) return ERR_STATE;
        for (int i = 0; i < N; ++i) shift[i] = b->data[i] * scale[i] + shift[i];
    }
    const int Np = (op.cout + 15) & ~15, Kp = kpad32(op.cin);
    op.w_off = pk.alloc((size_t)Np * Kp * 2);
    op.b_off = pk.alloc((size_t)Np * 4);
    uint16_t* W = (uint16_t*)(pk.blob.data() + op.w_off);
    float* Bv = (float*)(pk.blob.data() + op.b_off);
    for (int n = 0; n < N; ++n) {
        for (int k = 0; k < K; ++k) W[(size_t)n * Kp + k] = f2bf_host(w->data[(size_t)n * K + k] * scale[n]);
        Bv[n] = shift[n];
    }
    if (!op.ln_w_name.empty()) {   // LayerNorm folded into this GEMM (see Op::fuse_next)
        const TensorSpec* g = pk.get(op.ln_w_name);
        const TensorSpec* be = pk.get(op.ln_b_name);
        if (!g || !be) return ERR_STATE;
        MI355_REQUIRE(g->numel() == K && be->numel() == K, "pack: %s / %s must have %d elements", op.ln_w_name.c_str(),
                      op.ln_b_name.c_str(), K);
        op.w_ln_off = pk.alloc((size_t)Np * Kp * 2);
        op.b_ln_off = pk.alloc((size_t)Np * 4);
        op.cs_off = pk.alloc((size_t)Np * 4);
        uint16_t* W2 = (uint16_t*)(pk.blob.data() + op.w_ln_off);
        float* B2 = (float*)(pk.blob.data() + op.b_ln_off);
        float* CS = (float*)(pk.blob.data() + op.cs_off);
        const float* Bv1 = (const float*)(pk.blob.data() + op.b_off);     // (alloc may have moved the blob)
        for (int n = 0; n < N; ++n) {
            double cs = 0.0, bb = 0.0;
            for (int k = 0; k < K; ++k) {
                const float wv = w->data[(size_t)n * K + k] * scale[n];
                const uint16_t h = f2bf_host(wv * g->data[k]);
                W2[(size_t)n * Kp + k] = h;
                uint32_t u = (uint32_t)h << 16; float hf; memcpy(&hf, &u, 4);
                cs += hf;
                bb += (double)wv * be->data[k];
            }
            CS[n] = (float)cs;
            B2[n] = Bv1[n] + (float)bb;
        }
    }
    return OK;
}

static int pack_dw(Packer& pk, Op& op) {
    const TensorSpec* w = pk.get(op.w_name);
    if (!w) return ERR_STATE;
    const int C = op.cin_real, Cp = op.cin, kk = op.k * op.k;
    MI355_REQUIRE(w->numel() == (int64_t)C * kk, "pack: %s has %lld elements, expected %d x %d", op.w_name.c_str(),
                  (long long)w->numel(), C, kk);
    std::vector<float> scale, shift;
    if (!pk.bn_fold(op.bn_name, op.bn_eps, C, scale, shift)) return ERR_STATE;
    op.w_off = pk.alloc((size_t)kk * Cp * 2);
    op.b_off = pk.alloc((size_t)Cp * 4);
    uint16_t* W = (uint16_t*)(pk.blob.data() + op.w_off);
    float* Bv = (float*)(pk.blob.data() + op.b_off);
    for (int c = 0; c < C; ++c) {
        for (int t = 0; t < kk; ++t) W[(size_t)t * Cp + c] = f2bf_host(w->data[(size_t)c * kk + t] * scale[c]);
        Bv[c] = shift[c];
    }
    return OK;
}

static int pack_stem(Packer& pk, Op& op) {
    const TensorSpec* w = pk.get(op.w_name);
    if (!w) return ERR_STATE;
    const int Co = op.cout_real, Cp = op.cout;
    MI355_REQUIRE(w->numel() == (int64_t)Co * 27, "pack: %s has %lld elements, expected %d x 27", op.w_name.c_str(),
                  (long long)w->numel(), Co);
    std::vector<float> scale, shift;
    if (!pk.bn_fold(op.bn_name, op.bn_eps, Co, scale, shift)) return ERR_STATE;
    op.w_off = pk.alloc((size_t)27 * Cp * 4);
    op.b_off = pk.alloc((size_t)Cp * 4);
    float* W = (float*)(pk.blob.data() + op.w_off);
    float* Bv = (float*)(pk.blob.data() + op.b_off);
    for (int co = 0; co < Co; ++co) {
        for (int ci = 0; ci < 3; ++ci)
            for (int ky = 0; ky < 3; ++ky)
                for (int kx = 0; kx < 3; ++kx)
                    W[(size_t)((ky * 3 + kx) * 3 + ci) * Cp + co] =
                        bf_round_host(w->data[(((size_t)co * 3 + ci) * 3 + ky) * 3 + kx] * scale[co]);
        Bv[co] = shift[co];
    }
    return OK;
}

static int pack_se(Packer& pk, Op& op) {
    const TensorSpec *w1 = pk.get(op.w_name), *b1 = pk.get(op.bias_name), *w2 = pk.get(op.w2_name),
                     *b2 = pk.get(op.bias2_name);
    if (!w1 || !b1 || !w2 || !b2) return ERR_STATE;
    const int C = op.cin_real, Cp = op.cin, rd = op.rd;
    MI355_REQUIRE(w1->numel() == (int64_t)rd * C && w2->numel() == (int64_t)C * rd, "pack: SE %s shape mismatch",
                  op.w_name.c_str());
    std::vector<float> scale, shift;  // rexnet: BN between the reduce FC and its ReLU
    if (!pk.bn_fold(op.bn2_name, op.bn_eps, rd, scale, shift)) return ERR_STATE;
    op.w_off = pk.alloc((size_t)rd * Cp * 4);
    op.b_off = pk.alloc((size_t)rd * 4);
    op.w2_off = pk.alloc((size_t)Cp * rd * 4);
    op.b2_off = pk.alloc((size_t)Cp * 4);
    float* W1 = (float*)(pk.blob.data() + op.w_off);
    float* B1 = (float*)(pk.blob.data() + op.b_off);
    float* W2 = (float*)(pk.blob.data() + op.w2_off);
    float* B2 = (float*)(pk.blob.data() + op.b2_off);
    for (int j = 0; j < rd; ++j) {
        for (int c = 0; c < C; ++c) W1[(size_t)j * Cp + c] = bf_round_host(w1->data[(size_t)j * C + c] * scale[j]);   // bf16 values (see below)
        B1[j] = b1->data[j] * scale[j] + shift[j];
    }
    for (int c = 0; c < C; ++c) {
        for (int j = 0; j < rd; ++j) W2[(size_t)j * Cp + c] = bf_round_host(w2->data[(size_t)c * rd + j]);   // transposed [rd][Cp]
        B2[c] = b2->data[c];
    }
    // bf16 copies for the whole-block kernel (every workgroup streams both matrices from L2: half the bytes).  The fp32
    // copies above hold the same bf16-rounded values, so k_se and the block kernel compute the same gate.
    op.w3_off = pk.alloc((size_t)rd * Cp * 2);
    op.w4_off = pk.alloc((size_t)rd * Cp * 2);
    {
        // (alloc may have moved the blob: re-derive the fp32 views)
        const float* W1f = (const float*)(pk.blob.data() + op.w_off);
        const float* W2f = (const float*)(pk.blob.data() + op.w2_off);
        uint16_t* W1b = (uint16_t*)(pk.blob.data() + op.w3_off);
        uint16_t* W2b = (uint16_t*)(pk.blob.data() + op.w4_off);
        for (size_t i = 0; i < (size_t)rd * Cp; ++i) { W1b[i] = f2bf_host(W1f[i]); W2b[i] = f2bf_host(W2f[i]); }
    }
    return OK;
}

int swin_pack(Packer& pk, Op& op);  // swin_kernels.hip

static int pack_op(Packer& pk, Op& op) {
    switch (op.kind) {
        case OP_STEM: return pack_stem(pk, op);
        case OP_GEMM: return pack_gemm(pk, op);
        case OP_DW: return pack_dw(pk, op);
        case OP_SE: return pack_se(pk, op);
        default: return swin_pack(pk, op);
    }
}

// ------------------------------------------------------------------------------------ launch plan
static inline int conv_out(int h, int k, int s) { return (h + 2 * (k / 2) - k) / s + 1; }

// The one shape rule.  Returns the dims of what `op` writes given the dims `in` of what it reads (Step::in), and reports
// through need(slot, bytes) the arena bytes a chunk of nb images needs for it.
template <class Need>
static Dims op_shape(const Op& op, Dims in, int nb, int B_full, Need&& need) {
    Dims o = in;
    switch (op.kind) {
        case OP_STEM:
            o = {conv_out(in.h, 3, 2), conv_out(in.w, 3, 2), op.cout};
            break;
        case OP_GEMM:
            o.c = op.cout;
            // the caller's whole batch decides the kernel choices that change rounding (split-K); the chunk sizes the scratch
            if (gemm_splitk_chunks((long)B_full * in.h * in.w, in.h * in.w, op.cout, op.cin) >= 2)
                need(SLOT_SPLITK, gemm_splitk_bytes((long)nb * in.h * in.w, op.cout, op.cin));
            break;
        case OP_DW:
            o = {conv_out(in.h, op.k, op.stride), conv_out(in.w, op.k, op.stride), op.cout};
            // squeeze partials: per 256-item block (k_dwconv) or per row band (fused kernels, <= ho bands)
            if (op.pool) need(SLOT_POOLPART, (size_t)nb * std::max(dw_pool_blocks(o.h, o.w, op.cout), o.h) * op.cout * 4);
            break;
        case OP_SE:
            need(SLOT_GATE, (size_t)nb * op.cin * 4);
            return {1, 1, op.cin};
        default:
            // swin ops: sizes are declared by the builder through cin/cout/tokens_h
            o = {op.tokens_h, op.tokens_h, op.cout};
            if (op.kind == OP_LAYERNORM && op.fuse_next) need(SLOT_LNSTATS, (size_t)nb * op.tokens_h * op.tokens_h * 8);
            break;
    }
    need(op.out, (size_t)nb * o.h * o.w * o.c * 2);
    return o;
}

// The shape-only part of fused_pair_how: which fused front-half kernel takes an expand (cin -> mid, act_e) + depthwise (k, stride,
// act_d) pair on an h x w map under the options fuse_sweep / fuse_band (MI355_PLAN_FUSED_LATE / _SWEEP / _BAND), or
// MI355_PLAN_OP.  The launch plan and the developer entry mi355_mbconv_front_ex both decide here.
static int fused_pair_shape_how(int fuse_sweep, int fuse_band, int h, int w, int cin, int mid, int k, int stride, int act_e,
                                int act_d, int* band_rows) {
    if (fused_late_supported(h, w, cin, mid, k, stride)) return MI355_PLAN_FUSED_LATE;   // whole-image tile
    // row-sweep kernel (MFMA depthwise, complete squeeze sums): the early-stage shape classes of sweep_mbconv.hip
    if (fuse_sweep && sweep_mbconv_supported(h, w, cin, mid, k, stride, act_e, act_d)) return MI355_PLAN_SWEEP;
    // Band variant, measured per layer on EfficientNet-B3a B=256 (fused vs expand + depthwise): 3x3 s1 C192 @56x56 307 vs
    // 339 us (wins); 3x3 s2 C144 @112x112 780 vs 619, 5x5 s2 C192 @56x56 465 vs 276, 5x5 s1 C288 @28x28 247 vs 172 (lose:
    // short bands recompute too much halo and leave most threads idle in the depthwise phase).
    // RexNet-200: 3x3 s1 C324 @56x56 (7-row bands) 582 vs 661 us and 3x3 s2 C192 @112x112 714 vs 771 us (win: its 32->192
    // expand alone costs 0.5 ms).
    const int rows = fuse_band ? fused_band_rows(h, w, cin, mid, k, stride) : 0;
    const bool measured_win = k == 3 && ((stride == 1 && rows >= 7) || (stride == 2 && w >= 112 && mid >= 192));
    if (rows > 0 && (fuse_band == 1 || measured_win)) { *band_rows = rows; return MI355_PLAN_BAND; }
    return MI355_PLAN_OP;
}

// expand GEMM (-> SLOT_E) immediately followed by the depthwise conv that consumes it: which kernel runs the pair as one
// launch (MI355_PLAN_FUSED_LATE / _SWEEP / _BAND), or MI355_PLAN_OP when the two run apart
static int fused_pair_how(const mi355_model* m, size_t i, int h, int w, int* band_rows) {
    if (!m->fuse || i + 1 >= m->def.ops.size()) return MI355_PLAN_OP;
    const Op& g = m->def.ops[i];
    const Op& d = m->def.ops[i + 1];
    if (g.kind != OP_GEMM || d.kind != OP_DW || g.out != SLOT_E || d.in != SLOT_E) return MI355_PLAN_OP;
    if (g.use_gate || g.res != SLOT_NONE || g.a_relu6 || !g.tap.empty()) return MI355_PLAN_OP;
    return fused_pair_shape_how(m->fuse_sweep, m->fuse_band, h, w, g.cin, g.cout, d.k, d.stride, g.act, d.act, band_rows);
}

// expand GEMM -> depthwise -> SE -> gated projection on a whole-image tile: one kernel (mbconv_block.hip)
static bool can_fuse_block(const mi355_model* m, size_t i, int h, int w, int nb) {
    if (!m->fuse_block || nb < m->fuse_block_min_batch || i + 3 >= m->def.ops.size()) return false;
    const Op& g = m->def.ops[i];
    const Op& d = m->def.ops[i + 1];
    const Op& s = m->def.ops[i + 2];
    const Op& p = m->def.ops[i + 3];
    if (g.kind != OP_GEMM || d.kind != OP_DW || s.kind != OP_SE || p.kind != OP_GEMM) return false;
    if (g.out != SLOT_E || d.in != SLOT_E || d.out != SLOT_D || p.in != SLOT_D || !p.use_gate || !d.pool) return false;
    if (g.use_gate || g.res != SLOT_NONE || g.a_relu6 || !g.tap.empty() || !d.tap.empty()) return false;
    // (rexnet: ReLU6 behind the gate, a shortcut over the first res_channels outputs and channel counts padded to 8 are all
    //  handled by the kernel: pad channels carry exact zeros through every phase, as in the unfused chain)
    if (p.act != ACT_NONE || (p.res != SLOT_NONE && p.res != g.in)) return false;
    if (p.res != SLOT_NONE && p.res_channels && ((p.res_channels + 7) & ~7) != g.cin) return false;
    return mbconv_block_supported(h, w, g.cin, g.cout, p.cout, d.k, d.stride, s.rd, g.act, d.act);
}

// Pooled embedding wanted and the last op is the head 1x1 conv: conv + bias + act + GAP as ONE kernel (k_head_gap: the
// head tensor never reaches HBM).  forward_features, taps and per-op profiling need the un-pooled map: two-kernel path.
static bool can_fuse_head_gap(const mi355_model* m, size_t i, Dims in, bool pooled) {
    const ModelDef& d = m->def;
    if (!pooled || d.pools_in_features || !m->fuse_head_gap || m->taps || m->profile || i + 1 != d.ops.size()) return false;
    const Op& h = d.ops[i];
    if (h.kind != OP_GEMM || h.out != d.final_slot || h.in == SLOT_NONE || h.use_gate || h.res != SLOT_NONE || h.a_relu6 ||
        !h.ln_w_name.empty())
        return false;
    return head_gap_supported(in.h * in.w, h.cout, h.cin, h.cin, kpad32(h.cin), h.act);
}

struct PlanSeed {       // run_between_taps: the caller's activation sits in `slot` in front of the first op
    int slot = SLOT_NONE;
    Dims dims;
};

// The launch plan of ops [first_op, last_op] for a chunk of nb images of a batch of B_full: one walk over def.ops gives every
// op its shapes, sizes and lays out the arena slots (always for the whole op list, so a sub-range runs in the arena of a
// forward), and decides per step which kernel runs it.  This is the ONLY place a kernel is chosen; the executor, the
// profile and the traffic model walk the result.  `pooled`: the caller wants the pooled embedding, not the feature map.
static Plan resolve_plan(const mi355_model* m, size_t first_op, size_t last_op, PlanSeed seed, int nb, int B_full, int H, int W,
                         bool pooled) {
    const std::vector<Op>& ops = m->def.ops;
    Plan p;
    p.op_in.resize(ops.size());
    Dims D[SLOT_COUNT];
    auto need = [&](int s, size_t bytes) { if (s != SLOT_NONE && bytes > p.slots[s].bytes) p.slots[s].bytes = bytes; };
    size_t next = first_op;      // first op behind the steps resolved so far
    int ln_in = SLOT_NONE;       // a MI355_PLAN_LN_STATS step waits for its consumer GEMM: the slot that LayerNorm read
    for (size_t i = 0; i < ops.size(); ++i) {
        const Op& op = ops[i];
        if (i == first_op && seed.slot != SLOT_NONE) D[seed.slot] = seed.dims;
        // (the SE gate is computed from the squeeze partials of the depthwise conv in front of it: SLOT_D's geometry)
        const Dims in = op.in == SLOT_NONE ? Dims{H, W, 3} : D[op.kind == OP_SE ? SLOT_D : op.in];
        p.op_in[i] = in;
        // (a fused step never writes its SLOT_E; sizing it anyway keeps the arena as it was - a memory change of its own)
        const Dims out = op_shape(op, in, nb, B_full, need);
        if (op.out != SLOT_NONE) D[op.out] = out;
        if (i == next && i <= last_op) {
            Step s;
            s.first_op = (int)i;
            s.in = in;
            // (the whole-block kernel is chosen by the caller's WHOLE batch, not by the chunk: it rounds differently from the unfused chain)
            if (op.in != SLOT_NONE && can_fuse_block(m, i, in.h, in.w, B_full)) {
                s.how = MI355_PLAN_BLOCK;
                s.n_ops = 4;       // depthwise, SE and projection run inside the block kernel
            } else if ((s.how = fused_pair_how(m, i, in.h, in.w, &s.band_rows)) != MI355_PLAN_OP) {
                s.n_ops = 2;       // the depthwise op runs together with the expand
            } else if (can_fuse_head_gap(m, i, in, pooled)) {
                s.how = MI355_PLAN_HEAD_GAP;
            } else if (op.kind == OP_LAYERNORM) {
                // Folded into the next GEMM (norm1 -> qkv, norm2 -> fc1) when that GEMM takes the DMA-tiled kernel, whose epilogue
                // knows how (M >= 1024 rows of THIS chunk; smaller problems keep the separate kernel and the unfolded weights)
                // (and only where that epilogue exists: K >= 128 and a multiple of 64, so swin_s3's width-96 stage keeps the separate kernel).
                // SLOT_LNSTATS holds the rows * 8 bytes: op_shape sizes it to nb * tokens^2 * 8 for every fuse_next LayerNorm, in
                // this walk or, for a tail chunk, in the walk of the larger chunk whose slots the forward lays out.
                const long rows = (long)nb * op.tokens_h * op.tokens_h;
                if (op.fuse_next && m->fuse_ln && rows >= 1024 && op.cout >= 128 && op.cout % 64 == 0) {
                    s.how = MI355_PLAN_LN_STATS;
                    ln_in = op.in;
                }
            } else if (op.kind == OP_GEMM) {
                s.res_c = op.res != SLOT_NONE ? D[op.res].c : 0;
                s.ln_in = ln_in;
                ln_in = SLOT_NONE;
            }
            next = i + s.n_ops;
            p.steps.push_back(s);
        }
        if (i >= first_op && i < next) p.steps.back().out = out;   // the step's last op leaves its dims
    }
    p.final = D[m->def.final_slot];
    need(SLOT_POOLED, (size_t)nb * m->def.feat_dim_pad * 4);
    need(SLOT_POOLED_BF16, (size_t)nb * m->def.feat_dim_pad * 2);
    size_t off = 0;
    for (int i = 0; i < SLOT_COUNT; ++i) {
        p.slots[i].off = off;
        off += align_up(p.slots[i].bytes, 256);
    }
    p.arena_bytes = off + 256;
    return p;
}

static int ensure_arena(mi355_model* m, const Plan& plan, int lanes) {
    std::copy(plan.slots, plan.slots + SLOT_COUNT, m->slots);
    m->lane_bytes = lanes > 1 ? align_up(plan.arena_bytes, 4096) : 0;
    const size_t bytes = lanes > 1 ? m->lane_bytes * lanes : plan.arena_bytes;
    int dev = 0;
    MI355_CHECK_HIP(hipGetDevice(&dev));
    if (m->arena && m->arena_device != dev) {      // the model moved to another GPU: its scratch must follow
        MI355_CHECK_HIP(hipDeviceSynchronize());
        (void)hipFree(m->arena);                   // (hipFree finds the owning device by itself)
        m->arena = nullptr;
        m->arena_bytes = 0;
        for (auto& kv : m->tapbufs) { if (kv.second.ptr) (void)hipFree(kv.second.ptr); kv.second = TapBuf(); }
        if (m->stamp_buf) { (void)hipFree(m->stamp_buf); m->stamp_buf = nullptr; m->stamp_bytes = 0; }
    }
    m->arena_device = dev;
    if (bytes <= m->arena_bytes) return OK;
    if (m->arena) {
        MI355_CHECK_HIP(hipDeviceSynchronize());
        MI355_CHECK_HIP(hipFree(m->arena));
        m->arena = nullptr;
        m->arena_bytes = 0;
    }
    MI355_CHECK_HIP(hipMalloc(&m->arena, bytes));
    m->arena_bytes = bytes;
    return OK;
}

// ------------------------------------------------------------------------------------ labels, traffic model
static int prof_kind(const Op& op) {
    switch (op.kind) {
        case OP_STEM: return PK_STEM;
        case OP_GEMM: return PK_GEMM;
        case OP_DW: return PK_DW;
        case OP_SE: return PK_SE;
        case OP_WINATTN: return PK_ATTN;
        case OP_LAYERNORM: case OP_PATCH_MERGE_LN: case OP_TOKEN_MEAN: return PK_LN;
        case OP_PATCH_EMBED: return PK_STEM;
        default: return PK_OTHER;
    }
}

// Label, algorithmic HBM bytes and MACs of one op at batch B, from the op and the dims it reads.  Layer-granular model
// (SURVEY §8d): every conv/dw/1x1 layer reads its input once and writes its output once; BN/act/SE-gate/GAP are epilogues;
// each residual adds one read of the block input.
struct OpCost {
    char label[128];
    double bytes, macs;
    double table_bytes;     // what mi355_model_profile_ops reports: `bytes`, except for the discrepancy marked below
};
static OpCost op_cost(const Op& op, Dims in, int B) {
    OpCost c{};
    switch (op.kind) {
        case OP_STEM: {
            const int ho = conv_out(in.h, 3, 2), wo = conv_out(in.w, 3, 2);
            c.bytes = (double)B * (3.0 * in.h * in.w * 4 + (double)ho * wo * op.cout_real * 2);
            c.macs = (double)B * ho * wo * op.cout_real * 27;
            snprintf(c.label, sizeof c.label, "stem 3->%d @%dx%d", op.cout_real, ho, wo);
            break;
        }
        case OP_GEMM: {
            const double hw = (double)in.h * in.w;
            double el = hw * (op.cin_real + op.cout_real);
            if (op.res != SLOT_NONE) el += hw * (op.res_channels ? op.res_channels : op.cout_real);
            c.bytes = B * el * 2;
            c.macs = B * hw * op.cin_real * op.cout_real;
            snprintf(c.label, sizeof c.label, "pw %d->%d @%dx%d%s%s", op.cin_real, op.cout_real, in.h, in.w,
                     op.use_gate ? " gate" : "", op.res != SLOT_NONE ? " res" : "");
            break;
        }
        case OP_DW: {
            const int ho = conv_out(in.h, op.k, op.stride), wo = conv_out(in.w, op.k, op.stride);
            c.bytes = (double)B * ((double)in.h * in.w + (double)ho * wo) * op.cin_real * 2;
            c.macs = (double)B * ho * wo * op.cin_real * op.k * op.k;
            snprintf(c.label, sizeof c.label, "dw k%d s%d C%d @%dx%d", op.k, op.stride, op.cin_real, in.h, in.w);
            break;
        }
        case OP_SE:
            c.macs = (double)B * 2.0 * op.cin_real * op.rd;
            snprintf(c.label, sizeof c.label, "se C%d rd%d", op.cin_real, op.rd);
            break;
        default: {
            const double t = (double)op.tokens_h * op.tokens_h;
            c.bytes = c.table_bytes = B * t * (op.cin_real + op.cout_real) * 2;
            // KNOWN DISCREPANCY: the traffic model counts the patch embedding's fp32 image and the token mean's
            // single read; the per-op table counts both ops like every other token op.  Both values are kept as they were.
            if (op.kind == OP_PATCH_EMBED) c.bytes = (double)B * (3.0 * in.h * in.w * 4 + t * op.cout_real * 2);
            else if (op.kind == OP_TOKEN_MEAN) c.bytes = B * t * op.cin_real * 2;
            if (op.kind == OP_WINATTN) c.macs = B * t * (double)(op.window * op.window) * op.cout_real * 2;   // QK^T + PV
            if (op.kind == OP_PATCH_EMBED) c.macs = B * t * 48.0 * op.cout_real;
            snprintf(c.label, sizeof c.label, "op%d C%d->%d t%d", (int)op.kind, op.cin_real, op.cout_real, op.tokens_h);
            return c;
        }
    }
    c.table_bytes = c.bytes;
    return c;
}

// ------------------------------------------------------------------------------------ execution
static int record_tap(ExecCtx& cx, const Op& op, Dims s) {
    mi355_model* m = cx.m;
    TapBuf& t = m->tapbufs[op.tap];
    const size_t per_img = (size_t)s.h * s.w * s.c * 2;
    const size_t bytes = per_img * cx.B;
    if (t.bytes < bytes) {
        if (t.ptr) MI355_CHECK_HIP(hipFree(t.ptr));
        MI355_CHECK_HIP(hipMalloc(&t.ptr, bytes));
        t.bytes = bytes;
    }
    t.B = cx.B; t.h = s.h; t.w = s.w; t.c = s.c; t.c_real = op.cout_real ? op.cout_real : s.c;
    MI355_CHECK_HIP(hipMemcpyAsync((char*)t.ptr + per_img * cx.b0, cx.slot_ptr(op.out), per_img * cx.nb,
                                   hipMemcpyDeviceToDevice, cx.st));
    return OK;
}

static int exec_op(ExecCtx& cx, const Op& op, const Step& s) {
    mi355_model* m = cx.m;
    switch (op.kind) {
        case OP_STEM:
            if (const U8Source* u = cx.u8)
                return launch_stem_u8(cx.x_u8(), u->h, u->w, u->fill, u->mean, u->stdv, u->conv_w,
                                      (const float*)cx.w(op.w_off), (const float*)cx.w(op.b_off),
                                      (bf16_t*)cx.slot_ptr(op.out), cx.nb, op.cout, op.act, cx.st, u->desc, cx.b0);
            return launch_stem(cx.x, (const float*)cx.w(op.w_off), (const float*)cx.w(op.b_off),
                               (bf16_t*)cx.slot_ptr(op.out), cx.nb, s.in.h, s.in.w, op.cout, op.act, cx.st);
        case OP_GEMM: {
            const int hw = s.in.h * s.in.w;
            GemmArgs a{};
            a.A = (const bf16_t*)cx.slot_ptr(op.in); a.lda = op.cin;
            a.W = (const bf16_t*)cx.w(op.w_off); a.ldw = kpad32(op.cin);
            a.bias = (const float*)cx.w(op.b_off);
            a.res = op.res != SLOT_NONE ? (const bf16_t*)cx.slot_ptr(op.res) : nullptr;
            a.ldr = s.res_c;
            a.res_n = op.res_channels ? op.res_channels : op.cout;
            a.gate = op.use_gate ? (const float*)cx.slot_ptr(SLOT_GATE) : nullptr;
            a.gate_ld = op.cin; a.rows_per_img = hw;
            a.out = cx.slot_ptr(op.out); a.ldo = op.cout; a.out_f32 = 0;
            a.M = cx.nb * hw; a.N = op.cout; a.K = op.cin;
            a.M_sel = (long)cx.B * hw;
            a.act = op.act; a.a_relu6 = op.a_relu6;
            a.zeros = (const bf16_t*)cx.w(0);
            if (s.ln_in != SLOT_NONE) {      // the preceding LayerNorm only left (mean, rstd) per row: fold it in here
                MI355_REQUIRE(op.w_ln_off && op.in != SLOT_NONE, "exec: GEMM after a fused LayerNorm has no folded weights");
                a.A = (const bf16_t*)cx.slot_ptr(s.ln_in);
                a.W = (const bf16_t*)cx.w(op.w_ln_off);
                a.bias = (const float*)cx.w(op.b_ln_off);
                a.ln_stats = (const float*)cx.slot_ptr(SLOT_LNSTATS);
                a.ln_colsum = (const float*)cx.w(op.cs_off);
            }
            if (m->slots[SLOT_SPLITK].bytes) {
                a.splitk_ws = (float*)cx.slot_ptr(SLOT_SPLITK);
                a.splitk_ws_bytes = m->slots[SLOT_SPLITK].bytes;
            }
            return launch_gemm_bf16(a, cx.st);
        }
        case OP_DW:
            return launch_dwconv((const bf16_t*)cx.slot_ptr(op.in), (const bf16_t*)cx.w(op.w_off),
                                 (const float*)cx.w(op.b_off), (bf16_t*)cx.slot_ptr(op.out),
                                 op.pool ? (float*)cx.slot_ptr(SLOT_POOLPART) : nullptr, cx.nb, s.in.h, s.in.w,
                                 op.cin, op.k, op.stride, op.act, &cx.pool_nblk, cx.st);
        case OP_SE:
            return launch_se((const float*)cx.slot_ptr(SLOT_POOLPART), cx.pool_nblk,
                             1.0f / (float)(s.in.h * s.in.w), (const float*)cx.w(op.w_off), (const float*)cx.w(op.b_off),
                             (const float*)cx.w(op.w2_off), (const float*)cx.w(op.b2_off),
                             (float*)cx.slot_ptr(SLOT_GATE), cx.nb, op.cin, op.rd, op.se_act, cx.st);
        default:
            return swin_exec(op, s, cx);
    }
}

// diagnosis buffer [ops][B][16] of cycle buckets (option "block_stamps"); *out stays null when the option is off
static int stamp_ptr(ExecCtx& cx, size_t oi, long long** out) {
    mi355_model* m = cx.m;
    *out = nullptr;
    if (!m->block_stamps) return OK;
    const size_t need = m->def.ops.size() * (size_t)cx.B * 16 * sizeof(long long);
    if (m->stamp_bytes < need) {
        if (m->stamp_buf) MI355_CHECK_HIP(hipFree(m->stamp_buf));
        MI355_CHECK_HIP(hipMalloc((void**)&m->stamp_buf, need));
        m->stamp_bytes = need;
    }
    m->stamp_B = cx.B;
    *out = m->stamp_buf + (oi * (size_t)cx.B + cx.b0) * 16;
    MI355_CHECK_HIP(hipMemsetAsync(*out, 0, (size_t)cx.nb * 16 * sizeof(long long), cx.st));
    return OK;
}

// The operands FusedArgs, SweepArgs and BlockArgs share: block input, expand and depthwise weights, depthwise output, shapes.
// (Ho x Wo: the depthwise output, which the block's projection keeps.)
template <class Args>
static Args front_half_args(const ExecCtx& cx, const Step& s) {
    const Op& g = cx.m->def.ops[s.first_op];
    const Op& d = cx.m->def.ops[s.first_op + 1];
    Args a{};
    a.X = (const bf16_t*)cx.slot_ptr(g.in);
    a.We = (const bf16_t*)cx.w(g.w_off); a.be = (const float*)cx.w(g.b_off);
    a.Wd = (const bf16_t*)cx.w(d.w_off); a.bd = (const float*)cx.w(d.b_off);
    a.D = (bf16_t*)cx.slot_ptr(d.out);
    a.H = s.in.h; a.W = s.in.w; a.Cin = g.cin; a.Kp = kpad32(g.cin); a.mid = g.cout;
    a.Ho = s.out.h; a.Wo = s.out.w; a.act_e = g.act; a.act_d = d.act;
    return a;
}

static int exec_block(ExecCtx& cx, const Step& st) {
    mi355_model* m = cx.m;
    const Op& d = m->def.ops[st.first_op + 1];
    const Op& s = m->def.ops[st.first_op + 2];
    const Op& p = m->def.ops[st.first_op + 3];
    BlockArgs a = front_half_args<BlockArgs>(cx, st);
    a.W1 = (const bf16_t*)cx.w(s.w3_off); a.b1 = (const float*)cx.w(s.b_off);
    a.W2 = (const bf16_t*)cx.w(s.w4_off); a.b2 = (const float*)cx.w(s.b2_off);
    a.Wp = (const bf16_t*)cx.w(p.w_off); a.bp = (const float*)cx.w(p.b_off);
    a.Y = (bf16_t*)cx.slot_ptr(p.out);
    a.Cout = p.cout; a.Kp2 = kpad32(p.cin); a.rd = s.rd;
    a.has_res = p.res != SLOT_NONE;
    a.res_n = p.res != SLOT_NONE ? (p.res_channels ? ((p.res_channels + 7) & ~7) : p.cout) : 0;
    a.a_relu6 = p.a_relu6;
    a.se_act = s.se_act;
    a.inv_hw = 1.0f / (float)(a.Ho * a.Wo);
    a.norot = m->block_norot;
    a.variant = m->block_variant;
    if (int e = stamp_ptr(cx, st.first_op, &a.stamps)) return e;
    return launch_mbconv_block(a, cx.nb, d.k, d.stride, cx.st);
}

// expand + depthwise as one launch; leaves the squeeze partials' count for the SE op behind it
template <class Args>
static Args fused_pair_args(const ExecCtx& cx, const Step& s) {
    Args a = front_half_args<Args>(cx, s);
    a.pool = cx.m->def.ops[s.first_op + 1].pool ? (float*)cx.slot_ptr(SLOT_POOLPART) : nullptr;
    return a;
}
static int exec_fused(ExecCtx& cx, const Step& s) {
    mi355_model* m = cx.m;
    const Op& d = m->def.ops[s.first_op + 1];
    if (s.how == MI355_PLAN_SWEEP) {
        SweepArgs a = fused_pair_args<SweepArgs>(cx, s);
        a.csplit_override = m->sweep_csplit; a.variant = m->sweep_variant; a.debug_skip = m->sweep_skip;
        if (int e = stamp_ptr(cx, s.first_op, &a.stamps)) return e;
        cx.pool_nblk = 1;
        return launch_sweep_mbconv(a, cx.nb, d.k, d.stride, cx.st);
    }
    FusedArgs a = fused_pair_args<FusedArgs>(cx, s);
    a.debug_skip = m->fuse_debug;
    if (s.how == MI355_PLAN_FUSED_LATE) {
        cx.pool_nblk = 1;
        return launch_fused_late(a, cx.nb, d.k, d.stride, cx.st);
    }
    a.TH = s.band_rows;
    cx.pool_nblk = cdiv(a.Ho, a.TH);
    return launch_fused_band(a, cx.nb, d.k, d.stride, cx.st);
}

static int exec_head_gap(ExecCtx& cx, const Op& h, const Step& s) {
    return launch_head_gap((const bf16_t*)cx.slot_ptr(h.in), h.cin, (const bf16_t*)cx.w(h.w_off), kpad32(h.cin),
                           (const float*)cx.w(h.b_off), (float*)cx.slot_ptr(SLOT_POOLED),
                           cx.want_logits ? (bf16_t*)cx.slot_ptr(SLOT_POOLED_BF16) : nullptr, cx.m->def.feat_dim_pad, cx.nb,
                           s.in.h * s.in.w, h.cout, h.cin, h.act, cx.st);
}

// roctx range label of one step: the per-op table's wording behind how the step runs
static void step_range_label(const Op& op, const Step& s, char* lab, size_t n) {
    if (s.how == MI355_PLAN_HEAD_GAP) { snprintf(lab, n, "embed/head 1x1 + global average pool"); return; }
    snprintf(lab, n, "embed/%s%s", s.how == MI355_PLAN_BLOCK ? "block: " : (s.fused() ? "fused: " : ""), op_cost(op, s.in, 0).label);
}

static int run_backbone(ExecCtx& cx, const Plan& plan) {
    mi355_model* m = cx.m;
    for (const Step& s : plan.steps) {
        const Op& op = m->def.ops[s.first_op];
        hipEvent_t e0 = nullptr, e1 = nullptr;
        if (m->profile) {
            MI355_CHECK_HIP(hipEventCreate(&e0));
            MI355_CHECK_HIP(hipEventCreate(&e1));
            MI355_CHECK_HIP(hipEventRecord(e0, cx.st));
        }
        {
            char lab[192] = "";
            if (roctx_active()) step_range_label(op, s, lab, sizeof lab);
            RoctxRange range(lab);
            int e;
            switch (s.how) {
                case MI355_PLAN_BLOCK: e = exec_block(cx, s); break;
                case MI355_PLAN_FUSED_LATE: case MI355_PLAN_SWEEP: case MI355_PLAN_BAND: e = exec_fused(cx, s); break;
                case MI355_PLAN_HEAD_GAP: e = exec_head_gap(cx, op, s); break;
                default: e = exec_op(cx, op, s); break;      // MI355_PLAN_OP, and MI355_PLAN_LN_STATS inside swin_exec
            }
            if (e) return e;
        }
        if (m->profile) {
            MI355_CHECK_HIP(hipEventRecord(e1, cx.st));
            m->prof_events.push_back({s.first_op, s.how, e0, e1});
        }
        // a block's tap sits on its projection; an expand + depthwise pair has none (fused_pair_how)
        const Op& t = m->def.ops[s.first_op + (s.how == MI355_PLAN_BLOCK ? 3 : 0)];
        if (m->taps && !t.tap.empty())
            if (int e = record_tap(cx, t, s.out)) return e;
    }
    return OK;
}

// pooled rows [nb][Dp] fp32 -> the caller's [nb][D]
static int copy_pooled_rows(float* dst, const float* pooled, int nb, int D, int Dp, hipStream_t st) {
    MI355_CHECK_HIP(hipMemcpy2DAsync(dst, (size_t)D * 4, pooled, (size_t)Dp * 4, (size_t)D * 4, nb, hipMemcpyDeviceToDevice, st));
    return OK;
}

static int forward_impl(mi355_model* m, const float* x, int B, int H, int W, float* out, float* pooled_out,
                        bool features_only, hipStream_t st, const U8Source* u8 = nullptr) {
    MI355_REQUIRE(m, "forward: null model");
    MI355_REQUIRE(m->packed, "forward: weights not packed (call mi355_model_pack after set_tensor)");
    MI355_REQUIRE((x || u8) && out, "forward: null input/output pointer");
    MI355_REQUIRE(B >= 1 && H >= 32 && W >= 32, "forward: bad shape B=%d H=%d W=%d", B, H, W);
    const ModelDef& d = m->def;
    if (d.pools_in_features) MI355_REQUIRE(H == 224 && W == 224, "forward: %s needs 224x224 input", d.arch.c_str());
    // Chunking.  "lanes" > 1: the batch is cut into that many chunks which run CONCURRENTLY on internal streams (forked from
    // and joined back into the caller's stream with events), each with its own copy of the arena: the early layers are
    // HBM-bound and the late ones VALU-bound, so two half-batches a few kernels apart keep both busy where one
    // batch alternates between them.  Results do not depend on the chunking: every kernel is batch-position invariant, and the two
    // kernel choices that round differently from their alternatives (whole-block kernel vs the unfused chain, split-K vs the serial
    // K loop) are decided by the caller's whole batch B, never by the chunk.  (They DO depend on B itself: an image embedded alone
    // and the same image inside a batch of 256 agree to bf16 rounding, not bit for bit - tests/test_effnet_gpu.py.)
    int nl = m->lanes;
    if (nl > 4) nl = 4;
    if (nl < 1 || B < 32 * nl || m->profile || m->taps) nl = 1;
    int mb = (m->microbatch > 0 && m->microbatch < B) ? m->microbatch : B;
    if (nl > 1) mb = (B + nl - 1) / nl;
    // one plan per distinct chunk size: the chunk's, whose slots lay out the arena, and the shorter tail's (steps only)
    const size_t last_op = d.ops.size() - 1;
    const Plan plan = resolve_plan(m, 0, last_op, {}, mb, B, H, W, !features_only);
    const Plan tail = B % mb ? resolve_plan(m, 0, last_op, {}, B % mb, B, H, W, !features_only) : Plan();
    if (int e = ensure_arena(m, plan, nl)) return e;
    if (nl > 1) {
        if (!m->lane_fork) MI355_CHECK_HIP(hipEventCreateWithFlags(&m->lane_fork, hipEventDisableTiming));
        for (int l = 0; l < nl; ++l) {
            if (!m->lane_stream[l]) MI355_CHECK_HIP(hipStreamCreateWithFlags(&m->lane_stream[l], hipStreamNonBlocking));
            if (!m->lane_join[l]) MI355_CHECK_HIP(hipEventCreateWithFlags(&m->lane_join[l], hipEventDisableTiming));
        }
        MI355_CHECK_HIP(hipEventRecord(m->lane_fork, st));
    }
    hipStream_t caller_st = st;
    int lane = 0;
    const int D = d.feat_dim, Dp = d.feat_dim_pad;
    const bool want_logits = !features_only && d.num_classes > 0;
    for (int b0 = 0; b0 < B; b0 += mb, ++lane) {
        const int nb = std::min(mb, B - b0);
        const Plan& cp = nb == mb ? plan : tail;
        if (nl > 1) {
            st = m->lane_stream[lane];
            MI355_CHECK_HIP(hipStreamWaitEvent(st, m->lane_fork, 0));
        }
        ExecCtx cx{m, st, nb, x ? x + (size_t)b0 * 3 * H * W : nullptr, b0, B, u8};
        cx.lane = nl > 1 ? lane : 0;
        cx.want_logits = want_logits;
        if (int e = run_backbone(cx, cp)) return e;
        float* pooled = (float*)cx.slot_ptr(SLOT_POOLED);   // [nb][Dp]; swin: written by the final op, with its bf16 copy
        if (!d.pools_in_features) {
            const int hw = cp.final.h * cp.final.w;
            if (features_only)
                if (int e = launch_nhwc_to_nchw_f32((const bf16_t*)cx.slot_ptr(d.final_slot), out + (size_t)b0 * D * hw, nb, hw,
                                                    cp.final.c, D, st))
                    return e;
            if ((!features_only || pooled_out) && cp.steps.back().how != MI355_PLAN_HEAD_GAP)
                if (int e = launch_gap((const bf16_t*)cx.slot_ptr(d.final_slot), pooled,
                                       want_logits ? (bf16_t*)cx.slot_ptr(SLOT_POOLED_BF16) : nullptr, nb, hw, cp.final.c, st))
                    return e;
        }
        if ((d.pools_in_features || !features_only) && !want_logits)
            if (int e = copy_pooled_rows(out + (size_t)b0 * D, pooled, nb, D, Dp, st)) return e;
        if (pooled_out)
            if (int e = copy_pooled_rows(pooled_out + (size_t)b0 * D, pooled, nb, D, Dp, st)) return e;
        if (want_logits) {
            const Op& c = d.classifier;
            GemmArgs a{};
            a.A = (const bf16_t*)cx.slot_ptr(SLOT_POOLED_BF16); a.lda = Dp;
            a.W = (const bf16_t*)cx.w(c.w_off); a.ldw = kpad32(c.cin);
            a.bias = (const float*)cx.w(c.b_off);
            a.out = out + (size_t)b0 * d.num_classes; a.ldo = d.num_classes; a.out_f32 = 1;
            a.M = nb; a.N = d.num_classes; a.K = c.cin; a.act = ACT_NONE; a.rows_per_img = 1; a.res_n = a.N;
            a.zeros = (const bf16_t*)cx.w(0);
            if (int e = launch_gemm_bf16(a, st)) return e;
        }
        if (nl > 1) {
            MI355_CHECK_HIP(hipEventRecord(m->lane_join[lane], st));
            MI355_CHECK_HIP(hipStreamWaitEvent(caller_st, m->lane_join[lane], 0));
        }
    }
    return OK;
}

}  // namespace mi355

// ====================================================================================== C ABI
extern "C" {

int mi355_model_create(const char* name, int num_classes, mi355_model_t* out) {
    MI355_REQUIRE(name && out, "model_create: null argument");
    MI355_REQUIRE(num_classes >= 0, "model_create: num_classes=%d must be >= 0", num_classes);
    mi355_model* m = new mi355_model();
    m->def.arch = name;
    m->def.num_classes = num_classes;
    const std::string n = name;
    int e;
    if (n == "efficientnet_b3a" || n == "efficientnet_b3") e = build_efficientnet_b3(m->def);
    else if (n == "rexnet_100") e = build_rexnet(m->def, 1.0);
    else if (n == "rexnet_130") e = build_rexnet(m->def, 1.3);
    else if (n == "rexnet_150") e = build_rexnet(m->def, 1.5);
    else if (n == "rexnet_200") e = build_rexnet(m->def, 2.0);
    else if (n == "swin_base_patch4_window7_224") e = build_swin_base(m->def);
    else if (n == "swin_s3_base_224") e = build_swin_s3_base(m->def);
    else {
        // same wording as the reference's guard (train/train.py:400)
        set_error("Unknown model name '%s'. Known: efficientnet_b3a, rexnet_100/130/150/200, swin_base_patch4_window7_224, swin_s3_base_224", name);
        e = ERR_ARG;
    }
    if (e) { delete m; return e; }
    *out = m;
    return OK;
}

void mi355_model_destroy(mi355_model_t m) {
    if (!m) return;
    if (m->dev_blob) (void)hipFree(m->dev_blob);
    if (m->arena) (void)hipFree(m->arena);
    if (m->stamp_buf) (void)hipFree(m->stamp_buf);
    for (int l = 0; l < 4; ++l) {
        if (m->lane_stream[l]) (void)hipStreamDestroy(m->lane_stream[l]);
        if (m->lane_join[l]) (void)hipEventDestroy(m->lane_join[l]);
    }
    if (m->lane_fork) (void)hipEventDestroy(m->lane_fork);
    for (auto& kv : m->tapbufs)
        if (kv.second.ptr) (void)hipFree(kv.second.ptr);
    delete m;
}

int mi355_model_num_tensors(mi355_model_t m) { return m ? (int)m->def.tensors.size() : 0; }

int mi355_model_tensor_info(mi355_model_t m, int i, const char** name, int* ndim, int64_t shape[4], int* kind) {
    MI355_REQUIRE(m && i >= 0 && i < (int)m->def.tensors.size(), "tensor_info: index %d out of range", i);
    const TensorSpec& t = m->def.tensors[i];
    if (name) *name = t.name.c_str();
    if (ndim) *ndim = (int)t.shape.size();
    if (shape)
        for (int d = 0; d < 4; ++d) shape[d] = d < (int)t.shape.size() ? t.shape[d] : 1;
    if (kind) *kind = t.kind;
    return OK;
}

int mi355_model_feature_dim(mi355_model_t m) { return m ? m->def.feat_dim : 0; }
int mi355_model_num_classes(mi355_model_t m) { return m ? m->def.num_classes : 0; }

int mi355_model_set_tensor(mi355_model_t m, const char* name, const float* host_data, int64_t numel) {
    MI355_REQUIRE(m && name, "set_tensor: null argument");
    auto it = m->def.index.find(name);
    MI355_REQUIRE(it != m->def.index.end(), "set_tensor: unexpected key '%s' for %s", name, m->def.arch.c_str());
    TensorSpec& t = m->def.tensors[it->second];
    if (t.kind == 2) return OK;  // int64 buffers carry no arithmetic
    MI355_REQUIRE(host_data, "set_tensor: null data for '%s'", name);
    MI355_REQUIRE(numel == t.numel(), "set_tensor: size mismatch for '%s': got %lld elements, expected %lld", name,
                  (long long)numel, (long long)t.numel());
    t.data.assign(host_data, host_data + numel);
    t.set = true;
    m->packed = false;
    return OK;
}

int mi355_model_pack(mi355_model_t m, void* stream) {
    MI355_REQUIRE(m, "pack: null model");
    m->blob.clear();
    m->blob.resize(256, 0);   // zero page at offset 0 (source of out-of-range DMA chunks in k_gemm_big)
    Packer pk{m, m->blob};
    for (Op& op : m->def.ops)
        if (int e = pack_op(pk, op)) return e;
    if (m->def.num_classes > 0)
        if (int e = pack_gemm(pk, m->def.classifier)) return e;
    const size_t bytes = align_up(m->blob.size(), 256);
    m->blob.resize(bytes, 0);
    int dev = 0;
    MI355_CHECK_HIP(hipGetDevice(&dev));
    if (bytes > m->dev_blob_bytes || dev != m->blob_device) {   // (re-)allocate on the CURRENT device
        if (m->dev_blob) MI355_CHECK_HIP(hipFree(m->dev_blob));
        m->dev_blob = nullptr;
        MI355_CHECK_HIP(hipMalloc(&m->dev_blob, bytes));
        m->dev_blob_bytes = bytes;
        m->blob_device = dev;
    }
    hipStream_t st = (hipStream_t)stream;
    MI355_CHECK_HIP(hipMemcpyAsync(m->dev_blob, m->blob.data(), bytes, hipMemcpyHostToDevice, st));
    MI355_CHECK_HIP(hipStreamSynchronize(st));  // blob is pageable host memory
    m->packed = true;
    return OK;
}

int mi355_model_forward_features(mi355_model_t m, const float* x, int B, int H, int W, float* out, float* pooled_out,
                                 void* stream) {
    return forward_impl(m, x, B, H, W, out, pooled_out, true, (hipStream_t)stream);
}

int mi355_model_forward(mi355_model_t m, const float* x, int B, int H, int W, float* out, float* pooled_out,
                        void* stream) {
    return forward_impl(m, x, B, H, W, out, pooled_out, false, (hipStream_t)stream);
}

// Parity tool: run ONLY the ops behind tap `from_tap` up to and including the op that records tap `to_tap`, on an activation
// supplied by the caller (x: [B][C][h][w] fp32 NCHW, rounded to bf16 on the way in - feed it the oracle's bf16-rounded tap
// of the previous layer).  Taps are recorded as in a normal forward (enable them first), so each layer / block can be
// compared with the oracle on the ORACLE's input: errors do not compound through the network.
int mi355_model_run_between_taps(mi355_model_t m, const char* from_tap, const char* to_tap, const float* x, int B, int C,
                                 int h, int w, void* stream) {
    MI355_REQUIRE(m && from_tap && to_tap && x, "run_between_taps: null argument");
    MI355_REQUIRE(m->packed, "run_between_taps: weights not packed");
    MI355_REQUIRE(B >= 1 && C >= 1 && h >= 1 && w >= 1, "run_between_taps: bad shape");
    const auto& ops = m->def.ops;
    size_t i0 = ops.size(), i1 = ops.size();
    for (size_t i = 0; i < ops.size(); ++i) {
        if (ops[i].tap == from_tap) i0 = i;
        if (ops[i].tap == to_tap) i1 = i;
    }
    MI355_REQUIRE(i0 < ops.size() && i1 < ops.size() && i0 < i1, "run_between_taps: taps '%s' -> '%s' not found in that order",
                  from_tap, to_tap);
    const Op& src = ops[i0];
    MI355_REQUIRE(src.out != SLOT_NONE && (src.cout_real ? src.cout_real : src.cout) == C,
                  "run_between_taps: tap '%s' has %d channels, got %d", from_tap, src.cout_real ? src.cout_real : src.cout, C);
    hipStream_t st = (hipStream_t)stream;
    // size the arena as for a full forward whose input gives the tap this resolution: walk the strides in front of it
    int sh = 1;
    for (size_t i = 0; i <= i0; ++i)
        if (ops[i].kind == OP_STEM || (ops[i].kind == OP_DW && ops[i].stride == 2)) sh *= 2;
    const Plan plan = resolve_plan(m, i0 + 1, i1, {src.out, {h, w, src.cout}}, B, B, h * sh, w * sh, false);
    if (int e = ensure_arena(m, plan, 1)) return e;
    ExecCtx cx{m, st, B, nullptr, 0, B};
    if (int e = launch_nchw_f32_to_nhwc_bf16(x, (bf16_t*)cx.slot_ptr(src.out), B, h * w, C, src.cout, st)) return e;
    return run_backbone(cx, plan);
}

int mi355_model_forward_u8(mi355_model_t m, const unsigned char* images, int B, int h, int w, int fill, const float* mean,
                           const float* stdv, const float* conv_input_w, int features_only, float* out, float* pooled_out,
                           void* stream) {
    MI355_REQUIRE(m && images && mean && stdv && out, "forward_u8: null pointer");
    MI355_REQUIRE(B >= 1 && h >= 1 && w >= 1 && h <= 16384 && w <= 16384, "forward_u8: bad image size %dx%d", h, w);
    MI355_REQUIRE(fill >= 0 && fill <= 255, "forward_u8: fill must be a byte value");
    for (int c = 0; c < 3; ++c) MI355_REQUIRE(stdv[c] != 0.f, "forward_u8: std[%d] is zero", c);
    MI355_REQUIRE(!m->def.ops.empty() && (m->def.ops[0].kind == OP_STEM || m->def.ops[0].kind == OP_PATCH_EMBED),
                  "forward_u8: %s has no stem / patch embedding to fuse the pre-processing into", m->def.arch.c_str());
    MI355_REQUIRE(m->def.ops[0].kind == OP_STEM || !conv_input_w, "forward_u8: conv_input belongs to the convolutional backbones");
    U8Source u{};
    u.img = images; u.h = h; u.w = w; u.fill = fill; u.conv_w = conv_input_w;
    for (int c = 0; c < 3; ++c) { u.mean[c] = mean[c]; u.stdv[c] = stdv[c]; }
    const int S = h > w ? h : w;
    return forward_impl(m, nullptr, B, S, S, out, pooled_out, features_only != 0, (hipStream_t)stream, &u);
}

size_t mi355_model_forward_images_workspace_bytes(const int64_t* desc_host, int B, int transform, int out_size) {
    if (transform != 1 && transform != 2) return 0;     // "pad" needs none; anything else is refused by the forward
    const size_t rs = resize_batch_workspace(desc_host, B, out_size, out_size, transform == 2);
    return rs ? align_up((size_t)B * out_size * out_size * 3, 256) + rs : 0;
}

int mi355_model_forward_images(mi355_model_t m, const unsigned char* pixels, int64_t pixels_bytes, const int64_t* desc_host,
                               const int64_t* desc_dev, int B, int transform, int out_size, int fill, const float* mean,
                               const float* stdv, const float* conv_input_w, int features_only, float* out, float* pooled_out,
                               void* workspace, size_t workspace_bytes, void* stream) {
    MI355_REQUIRE(m && mean && stdv && out, "forward_images: null pointer");
    if (int e = check_images(pixels, pixels_bytes, desc_host, desc_dev, B, "forward_images")) return e;
    MI355_REQUIRE(transform >= 0 && transform <= 2, "forward_images: transform %d (0 = pad, 1 = resize, 2 = pad_resize)", transform);
    MI355_REQUIRE(fill >= 0 && fill <= 255, "forward_images: fill %d is not a byte value", fill);
    for (int c = 0; c < 3; ++c) MI355_REQUIRE(stdv[c] != 0.f, "forward_images: std[%d] is zero", c);
    MI355_REQUIRE(!m->def.ops.empty() && (m->def.ops[0].kind == OP_STEM || m->def.ops[0].kind == OP_PATCH_EMBED),
                  "forward_images: %s has no stem / patch embedding to fuse the pre-processing into", m->def.arch.c_str());
    const bool swin = m->def.ops[0].kind == OP_PATCH_EMBED;
    MI355_REQUIRE(!swin || !conv_input_w, "forward_images: conv_input belongs to the convolutional backbones");
    hipStream_t st = (hipStream_t)stream;
    U8Source u{};
    u.fill = fill; u.conv_w = conv_input_w;
    for (int c = 0; c < 3; ++c) { u.mean[c] = mean[c]; u.stdv[c] = stdv[c]; }
    if (transform == 0) {    // SquarePad in the stem's loads: one longer side for the whole batch (the reference's collate stacks)
        const int S = (int)std::max(desc_host[1], desc_host[2]);
        for (int b = 1; b < B; ++b)
            MI355_REQUIRE(std::max(desc_host[(size_t)b * 3 + 1], desc_host[(size_t)b * 3 + 2]) == S,
                          "forward_images: image %d has longer side %lld, image 0 has %d; \"pad\" needs one S per batch", b,
                          (long long)std::max(desc_host[(size_t)b * 3 + 1], desc_host[(size_t)b * 3 + 2]), S);
        MI355_REQUIRE(!swin || S == 224, "forward_images: swin needs images whose longer side is 224 (got %d)", S);
        MI355_REQUIRE(S >= 32, "forward_images: the longer side %d is below the backbone's 32", S);
        MI355_REQUIRE(m->packed, "forward_images: weights not packed (call mi355_model_pack after set_tensor)");
        u.img = pixels; u.desc = desc_dev; u.h = S; u.w = S;
        return forward_impl(m, nullptr, B, S, S, out, pooled_out, features_only != 0, st, &u);
    }
    MI355_REQUIRE(out_size >= 1 && out_size <= 16384, "forward_images: out_size %d outside 1..16384", out_size);
    MI355_REQUIRE(out_size >= 32, "forward_images: out_size %d is below the backbone's 32", out_size);
    MI355_REQUIRE(!swin || out_size == 224, "forward_images: swin needs out_size 224 (got %d)", out_size);
    const size_t need = mi355_model_forward_images_workspace_bytes(desc_host, B, transform, out_size);
    MI355_REQUIRE(workspace && workspace_bytes >= need, "forward_images: workspace of %zu bytes < %zu "
                  "(mi355_model_forward_images_workspace_bytes)", workspace_bytes, need);
    MI355_REQUIRE(m->packed, "forward_images: weights not packed (call mi355_model_pack after set_tensor)");
    // Resize into the head of the workspace, then the uniform uint8 forward (unchanged stem / patch embedding) on it
    unsigned char* resized = (unsigned char*)workspace;
    const size_t rbytes = align_up((size_t)B * out_size * out_size * 3, 256);
    if (int e = resize_batch(pixels, pixels_bytes, desc_host, desc_dev, B, out_size, out_size, transform == 2, fill, resized,
                             resized + rbytes, workspace_bytes - rbytes, st))
        return e;
    u.img = resized; u.h = out_size; u.w = out_size;
    return forward_impl(m, nullptr, B, out_size, out_size, out, pooled_out, features_only != 0, st, &u);
}

int mi355_model_enable_taps(mi355_model_t m, int enable) {
    MI355_REQUIRE(m, "enable_taps: null model");
    m->taps = enable != 0;
    return OK;
}

int mi355_model_read_tap(mi355_model_t m, const char* tap_name, float* out, int64_t out_numel, int64_t shape[4],
                         void* stream) {
    MI355_REQUIRE(m && tap_name, "read_tap: null argument");
    auto it = m->tapbufs.find(tap_name);
    MI355_REQUIRE(it != m->tapbufs.end(), "read_tap: no tap named '%s' was recorded", tap_name);
    const TapBuf& t = it->second;
    if (shape) { shape[0] = t.B; shape[1] = t.c_real; shape[2] = t.h; shape[3] = t.w; }
    if (!out) return OK;
    MI355_REQUIRE(out_numel >= (int64_t)t.B * t.c_real * t.h * t.w, "read_tap: output too small");
    return launch_nhwc_to_nchw_f32((const bf16_t*)t.ptr, out, t.B, t.h * t.w, t.c, t.c_real, (hipStream_t)stream);
}

int mi355_model_set_option(mi355_model_t m, const char* key, int64_t value) {
    MI355_REQUIRE(m && key, "set_option: null argument");
    const std::string k = key;
    if (k == "microbatch") m->microbatch = (int)value;
    else if (k == "lanes") m->lanes = (int)value;
    else if (k == "fuse") m->fuse = value != 0;
    else if (k == "fuse_band") m->fuse_band = (int)value;
    else if (k == "fuse_sweep") m->fuse_sweep = (int)value;
    else if (k == "sweep_csplit") m->sweep_csplit = (int)value;
    else if (k == "sweep_variant") m->sweep_variant = (int)value;
    else if (k == "sweep_skip") m->sweep_skip = (int)value;
    else if (k == "fuse_debug") m->fuse_debug = (int)value;
    else if (k == "fuse_ln") m->fuse_ln = (int)value;
    else if (k == "fuse_block") m->fuse_block = (int)value;
    else if (k == "fuse_block_min_batch") m->fuse_block_min_batch = (int)value;
    else if (k == "block_stamps") m->block_stamps = value != 0;
    else if (k == "block_norot") m->block_norot = (int)value;
    else if (k == "block_variant") m->block_variant = (int)value;
    else if (k == "fuse_head_gap") m->fuse_head_gap = value != 0;
    else if (k == "roctx") roctx_enable(value != 0);   // process-wide: ranges around every executor op and rank phase
    else if (k == "profile") {
        m->profile = value != 0;
        for (int i = 0; i < PK_COUNT; ++i) { m->prof_ms[i] = 0; m->prof_launches[i] = 0; }
        m->prof_op_ms.assign(m->def.ops.size(), 0.0);
        m->prof_op_n.assign(m->def.ops.size(), 0);
    } else {
        set_error("set_option: unknown option '%s'", key);
        return ERR_ARG;
    }
    return OK;
}

int mi355_model_profile_read(mi355_model_t m, double* ms_by_kind, int64_t* launches_by_kind, int n) {
    MI355_REQUIRE(m && ms_by_kind && launches_by_kind && n >= PK_COUNT, "profile_read: need arrays of >= %d", PK_COUNT);
    for (const ProfEvent& pe : m->prof_events) {
        MI355_CHECK_HIP(hipEventSynchronize(pe.e1));
        float ms = 0.f;
        MI355_CHECK_HIP(hipEventElapsedTime(&ms, pe.e0, pe.e1));
        const int kd = how_is_fused(pe.how) ? PK_FUSED : prof_kind(m->def.ops[pe.op]);
        m->prof_ms[kd] += ms;
        m->prof_launches[kd] += 1;
        if (m->prof_op_ms.size() < m->def.ops.size()) { m->prof_op_ms.resize(m->def.ops.size(), 0.0); m->prof_op_n.resize(m->def.ops.size(), 0); }
        m->prof_op_ms[pe.op] += ms;
        m->prof_op_n[pe.op] += 1;
        (void)hipEventDestroy(pe.e0);
        (void)hipEventDestroy(pe.e1);
    }
    m->prof_events.clear();
    for (int i = 0; i < PK_COUNT; ++i) { ms_by_kind[i] = m->prof_ms[i]; launches_by_kind[i] = m->prof_launches[i]; }
    return OK;
}

// Per-op view of the profile + traffic model: for op i (plan order) the average launch time (ms), its
// algorithmic bytes at batch B, its kind and a short label.  Call after mi355_model_profile_read.
int mi355_model_profile_ops(mi355_model_t m, int B, int H, int W, int max_ops, double* avg_ms, double* bytes,
                            int* kinds, char* labels, int label_stride) {
    MI355_REQUIRE(m && avg_ms && bytes && kinds, "profile_ops: null argument");
    const int n = (int)m->def.ops.size();
    MI355_REQUIRE(max_ops >= n, "profile_ops: need room for %d ops", n);
    const Plan plan = resolve_plan(m, 0, n - 1, {}, B, B, H, W, false);
    for (int i = 0; i < n; ++i) {
        const Op& op = m->def.ops[i];
        const OpCost c = op_cost(op, plan.op_in[i], B);
        avg_ms[i] = (i < (int)m->prof_op_n.size() && m->prof_op_n[i]) ? m->prof_op_ms[i] / m->prof_op_n[i] : 0.0;
        kinds[i] = prof_kind(op);
        bytes[i] = c.table_bytes;
        if (labels && label_stride > 0) { strncpy(labels + (size_t)i * label_stride, c.label, label_stride - 1); labels[(size_t)i * label_stride + label_stride - 1] = 0; }
    }
    return n;
}

// Layer-granular algorithmic traffic (op_cost) by kernel family; the ops of a step the executor runs as one fused kernel
// (expand + depthwise, whole block) count as PK_FUSED.
int mi355_model_traffic_kinds(mi355_model_t m, int B, int H, int W, double* bytes_by_kind, double* macs_by_kind, int n) {
    MI355_REQUIRE(m && bytes_by_kind && macs_by_kind && n >= PK_COUNT, "traffic_kinds: need arrays of >= %d", PK_COUNT);
    for (int i = 0; i < PK_COUNT; ++i) { bytes_by_kind[i] = 0; macs_by_kind[i] = 0; }
    const Plan plan = resolve_plan(m, 0, m->def.ops.size() - 1, {}, B, B, H, W, false);
    for (const Step& s : plan.steps)
        for (int i = s.first_op; i < s.first_op + s.n_ops; ++i) {
            const Op& op = m->def.ops[i];
            const OpCost c = op_cost(op, plan.op_in[i], B);
            const int kd = s.fused() ? PK_FUSED : prof_kind(op);
            bytes_by_kind[kd] += c.bytes;
            macs_by_kind[kd] += c.macs;
        }
    return OK;
}

static int plan_args_ok(mi355_model_t m, int B, int nb, int H, int W, int max_steps, const int* first_op, const int* n_ops,
                        const int* how, const size_t* arena_bytes) {
    MI355_REQUIRE(m && first_op && n_ops && how && arena_bytes && max_steps >= 0, "model_plan: null argument");
    MI355_REQUIRE(B >= 1 && nb >= 1 && nb <= B && H >= 32 && W >= 32, "model_plan: bad shape B=%d nb=%d H=%d W=%d", B, nb, H, W);
    return OK;
}

int mi355_model_plan(mi355_model_t m, int B, int nb, int H, int W, int pooled, int max_steps, int* first_op, int* n_ops,
                     int* how, size_t* arena_bytes) {
    if (int e = plan_args_ok(m, B, nb, H, W, max_steps, first_op, n_ops, how, arena_bytes)) return -e;
    const Plan plan = resolve_plan(m, 0, m->def.ops.size() - 1, {}, nb, B, H, W, pooled != 0);
    *arena_bytes = plan.arena_bytes;
    const int n = (int)plan.steps.size();
    for (int i = 0; i < n && i < max_steps; ++i) {
        first_op[i] = plan.steps[i].first_op; n_ops[i] = plan.steps[i].n_ops; how[i] = plan.steps[i].how;
    }
    return n;
}

int mi355_model_traffic(mi355_model_t m, int B, int H, int W, double* act_bytes, double* weight_bytes, double* macs) {
    MI355_REQUIRE(m, "traffic: null model");
    double by[PK_COUNT], mc[PK_COUNT];
    if (int e = mi355_model_traffic_kinds(m, B, H, W, by, mc, PK_COUNT)) return e;
    double tb = 0, tm = 0;
    for (int i = 0; i < PK_COUNT; ++i) { tb += by[i]; tm += mc[i]; }
    if (act_bytes) *act_bytes = tb;
    if (macs) *macs = tm;
    if (weight_bytes) *weight_bytes = (double)m->blob.size();
    return OK;
}

// Diagnosis: per-phase cycle counts of the whole-block kernel (option "block_stamps"), averaged over the images of the
// last forward.  out[op][16]: cycle buckets of wave 0 (the list is at the end of k_mbconv_block).
// Synchronises the device.  Returns the number of ops (rows) or a negative error.
int mi355_model_block_stamps(mi355_model_t m, double* out, int max_ops) {
    MI355_REQUIRE(m && out, "block_stamps: null argument");
    const int n = (int)m->def.ops.size();
    MI355_REQUIRE(max_ops >= n, "block_stamps: need room for %d ops", n);
    for (int i = 0; i < n * 16; ++i) out[i] = 0.0;
    if (!m->stamp_buf || m->stamp_B <= 0) return n;
    MI355_CHECK_HIP(hipDeviceSynchronize());
    std::vector<long long> h((size_t)n * m->stamp_B * 16);
    MI355_CHECK_HIP(hipMemcpy(h.data(), m->stamp_buf, h.size() * sizeof(long long), hipMemcpyDeviceToHost));
    for (int i = 0; i < n; ++i)
        for (int b = 0; b < m->stamp_B; ++b)
            for (int j = 0; j < 16; ++j) out[i * 16 + j] += (double)h[((size_t)i * m->stamp_B + b) * 16 + j] / m->stamp_B;
    return n;
}

// a 256-byte zero page per device: the source of the DMA kernels' out-of-range chunks (GemmArgs::zeros).  The one-time fill
// is enqueued on the caller's stream and finished before the pointer is published (as preprocess.hip::get_coeffs does): a
// memset on the null stream is not ordered before kernels on a non-blocking stream, and a later caller on ANOTHER stream must
// never find a page whose fill is still queued.
static int gemm_zero_page(const bf16_t** zeros, hipStream_t st) {
    static void* zero_page[MI355_MAX_DEVICES] = {nullptr};
    int dev = 0;
    MI355_CHECK_HIP(hipGetDevice(&dev));
    MI355_REQUIRE(dev >= 0 && dev < MI355_MAX_DEVICES, "gemm_bf16: device ordinal %d out of range", dev);
    if (!zero_page[dev]) {
        void* page = nullptr;
        MI355_CHECK_HIP(hipMalloc(&page, 256));
        MI355_CHECK_HIP(hipMemsetAsync(page, 0, 256, st));
        MI355_CHECK_HIP(hipStreamSynchronize(st));
        zero_page[dev] = page;
    }
    *zeros = (const bf16_t*)zero_page[dev];
    return OK;
}

int mi355_gemm_bf16(const void* A, const void* W, const float* bias, void* out, int M, int N, int K, int ldw, int act,
                    void* stream) {
    MI355_REQUIRE(A && W && bias && out, "gemm_bf16: null pointer");
    GemmArgs a{};
    a.A = (const bf16_t*)A; a.lda = K; a.W = (const bf16_t*)W; a.ldw = ldw; a.bias = bias;
    a.out = out; a.ldo = N; a.out_f32 = 0; a.M = M; a.N = N; a.K = K; a.act = act; a.rows_per_img = 1; a.res_n = N;
    if (int e = gemm_zero_page(&a.zeros, (hipStream_t)stream)) return e;
    return launch_gemm_bf16(a, (hipStream_t)stream);
}

int mi355_gemm_bf16_ex(const mi355_gemm_ex_args* x, int* path, void* stream) {
    if (path) *path = 0;
    MI355_REQUIRE(x, "gemm_bf16_ex: null argument block");
    MI355_REQUIRE(x->A && x->W && x->bias && x->out, "gemm_bf16_ex: null pointer");
    MI355_REQUIRE(x->M >= 1 && x->N >= 1 && x->K >= 1, "gemm_bf16_ex: bad shape M=%d N=%d K=%d", x->M, x->N, x->K);
    MI355_REQUIRE(x->K % 8 == 0 && x->lda >= x->K && x->lda % 8 == 0, "gemm_bf16_ex: K=%d lda=%d: K and lda multiples of 8, lda >= K",
                  x->K, x->lda);
    MI355_REQUIRE(x->ldw >= x->K && x->ldw % 32 == 0, "gemm_bf16_ex: ldw=%d must be a multiple of 32 and >= K=%d", x->ldw, x->K);
    MI355_REQUIRE(x->ldo >= x->N, "gemm_bf16_ex: ldo=%d < N=%d", x->ldo, x->N);
    MI355_REQUIRE(x->out_f32 || (x->N % 8 == 0 && x->ldo % 8 == 0), "gemm_bf16_ex: bf16 output needs N, ldo multiples of 8 (N=%d ldo=%d)",
                  x->N, x->ldo);
    MI355_REQUIRE(x->act >= ACT_NONE && x->act <= ACT_SIGMOID, "gemm_bf16_ex: unknown activation %d", x->act);
    MI355_REQUIRE(!x->res || (x->res_n >= 1 && x->res_n <= x->N && x->ldr >= x->res_n && x->ldr % 4 == 0),
                  "gemm_bf16_ex: residual needs 1 <= res_n <= N and ldr >= res_n, a multiple of 4 (res_n=%d ldr=%d)", x->res_n, x->ldr);
    MI355_REQUIRE(!x->gate || (x->gate_ld >= x->K && x->gate_ld % 4 == 0 && x->rows_per_img >= 1),
                  "gemm_bf16_ex: gate needs gate_ld >= K, a multiple of 4, and rows_per_img >= 1 (gate_ld=%d rows_per_img=%d)",
                  x->gate_ld, x->rows_per_img);
    MI355_REQUIRE(x->rows_per_img >= 0, "gemm_bf16_ex: bad rows_per_img %d", x->rows_per_img);
    MI355_REQUIRE(x->M_sel >= 0 && x->M_sel < (1ll << 31), "gemm_bf16_ex: bad M_sel %lld", (long long)x->M_sel);
    MI355_REQUIRE(!x->splitk_ws == !x->splitk_ws_bytes, "gemm_bf16_ex: split-K workspace and its size go together");
    MI355_REQUIRE(!x->ln_stats == !x->ln_colsum, "gemm_bf16_ex: ln_stats and ln_colsum go together");
    for (const void* p : {x->A, x->W, (const void*)x->bias, x->res, (const void*)x->gate, (const void*)x->out, (const void*)x->splitk_ws,
                          (const void*)x->ln_stats, (const void*)x->ln_colsum})
        MI355_REQUIRE((uintptr_t)p % 16 == 0, "gemm_bf16_ex: pointers must be 16-byte aligned");
    GemmArgs a{};
    a.A = (const bf16_t*)x->A; a.lda = x->lda; a.W = (const bf16_t*)x->W; a.ldw = x->ldw; a.bias = x->bias;
    a.res = (const bf16_t*)x->res; a.ldr = x->res ? x->ldr : 0; a.res_n = x->res ? x->res_n : x->N;
    a.gate = x->gate; a.gate_ld = x->gate ? x->gate_ld : 0; a.rows_per_img = x->rows_per_img;
    a.a_relu6 = x->a_relu6 ? 1 : 0;
    a.out = x->out; a.ldo = x->ldo; a.out_f32 = x->out_f32 ? 1 : 0;
    a.M = x->M; a.N = x->N; a.K = x->K; a.act = x->act;
    a.M_sel = (long)x->M_sel;
    a.splitk_ws = (float*)x->splitk_ws; a.splitk_ws_bytes = x->splitk_ws_bytes;
    a.ln_stats = x->ln_stats; a.ln_colsum = x->ln_colsum;
    if (int e = gemm_zero_page(&a.zeros, (hipStream_t)stream)) return e;
    return launch_gemm_bf16(a, (hipStream_t)stream, path);
}

int mi355_dwconv_se_ex(const mi355_dwconv_ex_args* x, int* path, void* stream) {
    if (path) *path = 0;
    MI355_REQUIRE(x, "dwconv_se_ex: null argument block");
    MI355_REQUIRE(x->in && x->w && x->bias && x->out, "dwconv_se_ex: null pointer");
    MI355_REQUIRE(x->B >= 1 && x->H >= 1 && x->W >= 1 && x->H <= 16384 && x->W <= 16384 && x->C >= 8,
                  "dwconv_se_ex: bad shape B=%d H=%d W=%d C=%d", x->B, x->H, x->W, x->C);
    MI355_REQUIRE(x->C % 8 == 0, "dwconv_se_ex: C=%d must be a multiple of 8", x->C);
    MI355_REQUIRE((size_t)x->B * x->H * x->W * x->C < ((size_t)1 << 36), "dwconv_se_ex: tensor too large");
    MI355_REQUIRE((x->k == 3 || x->k == 5) && (x->stride == 1 || x->stride == 2), "dwconv_se_ex: unsupported k=%d stride=%d",
                  x->k, x->stride);
    MI355_REQUIRE(x->act >= ACT_NONE && x->act <= ACT_SIGMOID, "dwconv_se_ex: unknown activation %d", x->act);
    MI355_REQUIRE(x->choice >= MI355_DW_CHOICE_AUTO && x->choice <= MI355_DW_CHOICE_MFMA, "dwconv_se_ex: unknown choice %d",
                  x->choice);
    MI355_REQUIRE(x->choice != MI355_DW_CHOICE_TILED || dw_tiled_supported(x->H, x->W, x->C, x->k, x->stride),
                  "dwconv_se_ex: choice tiled does not take H=%d W=%d C=%d k=%d stride=%d", x->H, x->W, x->C, x->k, x->stride);
    MI355_REQUIRE(x->choice != MI355_DW_CHOICE_MFMA || dw3_lds_supported(x->H, x->W, x->C, x->k, x->stride),
                  "dwconv_se_ex: choice mfma does not take H=%d W=%d C=%d k=%d stride=%d", x->H, x->W, x->C, x->k, x->stride);
    const bool se = x->se_w1 != nullptr;
    MI355_REQUIRE(!x->se_b1 == !se && !x->se_w2t == !se && !x->se_b2 == !se && !x->gate == !se,
                  "dwconv_se_ex: the SE weights, biases and gate go together");
    MI355_REQUIRE(!se || (x->rd >= 1 && x->rd <= SE_MAX_RD && x->C <= SE_MAX_C),
                  "dwconv_se_ex: SE needs 1 <= rd <= %d and C <= %d (rd=%d C=%d)", SE_MAX_RD, SE_MAX_C, x->rd, x->C);
    MI355_REQUIRE(!se || (x->act1 >= ACT_NONE && x->act1 <= ACT_SIGMOID), "dwconv_se_ex: unknown SE activation %d", x->act1);
    for (const void* p : {x->in, x->w, (const void*)x->bias, (const void*)x->out})
        MI355_REQUIRE((uintptr_t)p % 16 == 0, "dwconv_se_ex: in, w, bias and out must be 16-byte aligned");
    for (const void* p : {(const void*)x->se_w1, (const void*)x->se_b1, (const void*)x->se_w2t, (const void*)x->se_b2,
                          (const void*)x->gate, (const void*)x->squeeze})
        MI355_REQUIRE((uintptr_t)p % 4 == 0, "dwconv_se_ex: SE and squeeze pointers must be 4-byte aligned");
    const int Ho = (x->H - 1) / x->stride + 1, Wo = (x->W - 1) / x->stride + 1;
    bool try_tiled = x->choice == MI355_DW_CHOICE_TILED, try_mfma = x->choice == MI355_DW_CHOICE_MFMA;
    if (x->choice == MI355_DW_CHOICE_AUTO) dw_env_choice(&try_tiled, &try_mfma);
    // squeeze partials: at most dw_pool_blocks(...) per image (direct / matrix-pipe kernels) or one per row band (<= H)
    const size_t nblk_max = (size_t)std::max(dw_pool_blocks(Ho, Wo, x->C), x->H);
    float* partial = nullptr;
    MI355_CHECK_HIP(hipMalloc(&partial, nblk_max * x->B * x->C * sizeof(float)));
    const hipStream_t st = (hipStream_t)stream;
    int nblk = 0, dw_path = 0, se_path = 0;
    int e = launch_dwconv_sel((const bf16_t*)x->in, (const bf16_t*)x->w, x->bias, (bf16_t*)x->out, partial, x->B, x->H, x->W,
                              x->C, x->k, x->stride, x->act, try_tiled, try_mfma, &nblk, &dw_path, st);
    if (e == OK && se)
        e = launch_se(partial, nblk, 1.0f / (float)(Ho * Wo), x->se_w1, x->se_b1, x->se_w2t, x->se_b2, x->gate, x->B, x->C, x->rd,
                      x->act1, st, &se_path);
    hipError_t he = hipStreamSynchronize(st);
    std::vector<float> part, sq;
    if (e == OK && he == hipSuccess && x->squeeze) {
        // k_se's squeeze: the partials of one (image, channel) added in partial order, then one multiply
        const size_t n = (size_t)x->B * nblk * x->C;
        part.resize(n);
        sq.resize((size_t)x->B * x->C);
        he = hipMemcpy(part.data(), partial, n * sizeof(float), hipMemcpyDeviceToHost);
        const float inv_hw = 1.0f / (float)(Ho * Wo);
        for (int b = 0; b < x->B; ++b)
            for (int c = 0; c < x->C; ++c) {
                float a = 0.f;
                for (int k = 0; k < nblk; ++k) a += part[((size_t)b * nblk + k) * x->C + c];
                sq[(size_t)b * x->C + c] = a * inv_hw;
            }
        if (he == hipSuccess) he = hipMemcpy(x->squeeze, sq.data(), sq.size() * sizeof(float), hipMemcpyHostToDevice);
    }
    const hipError_t freed = hipFree(partial);
    if (e != OK) return e;
    MI355_CHECK_HIP(he);
    MI355_CHECK_HIP(freed);
    if (path) *path = dw_path | se_path << 24;
    return OK;
}

int mi355_mbconv_front_ex(const mi355_mbconv_front_args* x, int* pool_nblk, int* path, void* stream) {
    if (path) *path = 0;
    if (pool_nblk) *pool_nblk = 0;
    MI355_REQUIRE(x, "mbconv_front_ex: null argument block");
    MI355_REQUIRE(x->X && x->We && x->be && x->Wd && x->bd && x->D, "mbconv_front_ex: null pointer");
    MI355_REQUIRE(x->B >= 1 && x->B <= 65535 && x->H >= 1 && x->W >= 1 && x->H <= 16384 && x->W <= 16384 && x->Cin >= 8 && x->mid >= 8 &&
                      x->Cin <= 32768 && x->mid <= 32768,
                  "mbconv_front_ex: bad shape B=%d H=%d W=%d Cin=%d mid=%d", x->B, x->H, x->W, x->Cin, x->mid);
    MI355_REQUIRE(x->Cin % 8 == 0 && x->mid % 8 == 0, "mbconv_front_ex: Cin=%d and mid=%d must be multiples of 8", x->Cin, x->mid);
    MI355_REQUIRE((size_t)x->B * x->H * x->W * std::max(x->Cin, x->mid) < ((size_t)1 << 36), "mbconv_front_ex: tensor too large");
    MI355_REQUIRE((x->k == 3 || x->k == 5) && (x->stride == 1 || x->stride == 2), "mbconv_front_ex: unsupported k=%d stride=%d", x->k,
                  x->stride);
    MI355_REQUIRE(x->act_e >= ACT_NONE && x->act_e <= ACT_SIGMOID && x->act_d >= ACT_NONE && x->act_d <= ACT_SIGMOID,
                  "mbconv_front_ex: unknown activation %d / %d", x->act_e, x->act_d);
    MI355_REQUIRE(x->kernel >= MI355_FRONT_KERNEL_AUTO && x->kernel <= MI355_FRONT_KERNEL_BAND, "mbconv_front_ex: unknown kernel %d",
                  x->kernel);
    MI355_REQUIRE(x->band_rows >= 0 && x->sweep_variant >= 0 && x->sweep_variant <= 4 && x->sweep_csplit >= 0 && x->sweep_csplit <= 4095,
                  "mbconv_front_ex: band_rows=%d, sweep_variant=%d (0..4) or sweep_csplit=%d (0..4095) out of range", x->band_rows,
                  x->sweep_variant, x->sweep_csplit);
    for (const void* p : {x->X, x->We, (const void*)x->be, x->Wd, (const void*)x->bd, (const void*)x->D, (const void*)x->pool})
        MI355_REQUIRE((uintptr_t)p % 16 == 0, "mbconv_front_ex: pointers must be 16-byte aligned");
    const int H = x->H, W = x->W, Cin = x->Cin, mid = x->mid, k = x->k, stride = x->stride;
    int rows = 0, how = x->kernel;
    if (how == MI355_FRONT_KERNEL_AUTO) {
        const mi355_model defaults{};    // the options a fresh model has
        how = fused_pair_shape_how(defaults.fuse_sweep, defaults.fuse_band, H, W, Cin, mid, k, stride, x->act_e, x->act_d, &rows);
        MI355_REQUIRE(how != MI355_PLAN_OP, "mbconv_front_ex: the launch plan runs H=%d W=%d Cin=%d mid=%d k=%d stride=%d unfused", H, W,
                      Cin, mid, k, stride);
    }
    static_assert(MI355_FRONT_KERNEL_LATE == MI355_PLAN_FUSED_LATE && MI355_FRONT_KERNEL_SWEEP == MI355_PLAN_SWEEP &&
                      MI355_FRONT_KERNEL_BAND == MI355_PLAN_BAND, "the forced kinds are the plan's");
    MI355_REQUIRE(how != MI355_FRONT_KERNEL_LATE || fused_late_supported(H, W, Cin, mid, k, stride),
                  "mbconv_front_ex: kernel late does not take H=%d W=%d Cin=%d mid=%d k=%d stride=%d", H, W, Cin, mid, k, stride);
    MI355_REQUIRE(how != MI355_FRONT_KERNEL_SWEEP || (sweep_mbconv_supported(H, W, Cin, mid, k, stride, x->act_e, x->act_d) && kpad32(Cin) <= 128),
                  "mbconv_front_ex: kernel sweep does not take H=%d W=%d Cin=%d mid=%d k=%d stride=%d act %d / %d", H, W, Cin, mid, k,
                  stride, x->act_e, x->act_d);
    if (how == MI355_FRONT_KERNEL_BAND) {
        const int most = fused_band_rows(H, W, Cin, mid, k, stride);
        MI355_REQUIRE(most > 0 && kpad32(Cin) <= 64, "mbconv_front_ex: kernel band does not take H=%d W=%d Cin=%d mid=%d k=%d stride=%d", H, W,
                      Cin, mid, k, stride);
        MI355_REQUIRE(x->band_rows <= most, "mbconv_front_ex: band_rows=%d exceeds the %d rows that fit the LDS", x->band_rows, most);
        rows = x->band_rows ? x->band_rows : most;
    } else {
        MI355_REQUIRE(x->band_rows == 0, "mbconv_front_ex: band_rows belongs to the band kernel");
    }
    MI355_REQUIRE(how == MI355_FRONT_KERNEL_SWEEP || (x->sweep_variant == 0 && x->sweep_csplit == 0),
                  "mbconv_front_ex: sweep_variant and sweep_csplit belong to the sweep kernel");
    const int Ho = conv_out(H, k, stride), Wo = conv_out(W, k, stride);
    const hipStream_t st = (hipStream_t)stream;
    if (how == MI355_FRONT_KERNEL_SWEEP) {
        SweepArgs a{};
        a.X = (const bf16_t*)x->X; a.We = (const bf16_t*)x->We; a.be = x->be; a.Wd = (const bf16_t*)x->Wd; a.bd = x->bd;
        a.D = (bf16_t*)x->D; a.pool = x->pool;
        a.H = H; a.W = W; a.Cin = Cin; a.Kp = kpad32(Cin); a.mid = mid; a.Ho = Ho; a.Wo = Wo; a.act_e = x->act_e; a.act_d = x->act_d;
        a.csplit_override = x->sweep_csplit; a.variant = x->sweep_variant;
        if (pool_nblk) *pool_nblk = 1;
        return launch_sweep_mbconv(a, x->B, k, stride, st, path);
    }
    FusedArgs a{};
    a.X = (const bf16_t*)x->X; a.We = (const bf16_t*)x->We; a.be = x->be; a.Wd = (const bf16_t*)x->Wd; a.bd = x->bd;
    a.D = (bf16_t*)x->D; a.pool = x->pool;
    a.H = H; a.W = W; a.Cin = Cin; a.Kp = kpad32(Cin); a.mid = mid; a.Ho = Ho; a.Wo = Wo; a.act_e = x->act_e; a.act_d = x->act_d;
    if (how == MI355_FRONT_KERNEL_LATE) {
        if (pool_nblk) *pool_nblk = 1;
        return launch_fused_late(a, x->B, k, stride, st, path);
    }
    a.TH = rows;
    if (pool_nblk) *pool_nblk = cdiv(Ho, rows);
    return launch_fused_band(a, x->B, k, stride, st, path);
}

// the shape checks mi355_mbconv_block_ex and mi355_mbconv_block_how share (everything mbconv_block_supported takes for granted)
static int block_shape_check(const char* who, int H, int W, int Cin, int mid, int Cout, int k, int stride, int rd, int act_e, int act_d) {
    MI355_REQUIRE(H >= 1 && W >= 1 && H <= 16384 && W <= 16384 && Cin >= 8 && mid >= 8 && Cout >= 8 && Cin <= 32768 && mid <= 32768 &&
                      Cout <= 32768 && rd >= 1 && rd <= 32768,
                  "%s: bad shape H=%d W=%d Cin=%d mid=%d Cout=%d rd=%d", who, H, W, Cin, mid, Cout, rd);
    MI355_REQUIRE(Cin % 8 == 0 && mid % 8 == 0 && Cout % 8 == 0, "%s: Cin=%d, mid=%d and Cout=%d must be multiples of 8", who, Cin, mid, Cout);
    MI355_REQUIRE((k == 3 || k == 5) && (stride == 1 || stride == 2), "%s: unsupported k=%d stride=%d", who, k, stride);
    MI355_REQUIRE(act_e >= ACT_NONE && act_e <= ACT_SIGMOID && act_d >= ACT_NONE && act_d <= ACT_SIGMOID, "%s: unknown activation %d / %d",
                  who, act_e, act_d);
    return OK;
}

// BlockArgs as exec_block fills them, from a shape
static BlockArgs block_shape_args(int H, int W, int Cin, int mid, int Cout, int k, int stride, int rd, int act_e, int act_d) {
    BlockArgs a{};
    a.H = H; a.W = W; a.Cin = Cin; a.Kp = kpad32(Cin); a.mid = mid;
    a.Ho = conv_out(H, k, stride); a.Wo = conv_out(W, k, stride); a.act_e = act_e; a.act_d = act_d;
    a.Cout = Cout; a.Kp2 = kpad32(mid); a.rd = rd;
    a.inv_hw = 1.0f / (float)(a.Ho * a.Wo);
    return a;
}

int mi355_mbconv_block_how(int H, int W, int Cin, int mid, int Cout, int k, int stride, int rd, int act_e, int act_d, int* path) {
    if (path) *path = 0;
    if (int e = block_shape_check("mbconv_block_how", H, W, Cin, mid, Cout, k, stride, rd, act_e, act_d)) return e;
    return launch_mbconv_block(block_shape_args(H, W, Cin, mid, Cout, k, stride, rd, act_e, act_d), 1, k, stride, nullptr, path, true);
}

int mi355_mbconv_block_ex(const mi355_mbconv_block_args* x, int* path, void* stream) {
    if (path) *path = 0;
    MI355_REQUIRE(x, "mbconv_block_ex: null argument block");
    MI355_REQUIRE(x->X && x->We && x->be && x->Wd && x->bd && x->W1 && x->b1 && x->W2 && x->b2 && x->Wp && x->bp && x->D && x->Y,
                  "mbconv_block_ex: null pointer");
    MI355_REQUIRE(x->B >= 1 && x->B <= 65535, "mbconv_block_ex: bad shape B=%d", x->B);
    if (int e = block_shape_check("mbconv_block_ex", x->H, x->W, x->Cin, x->mid, x->Cout, x->k, x->stride, x->rd, x->act_e, x->act_d))
        return e;
    MI355_REQUIRE(x->se_act >= ACT_NONE && x->se_act <= ACT_SIGMOID, "mbconv_block_ex: unknown SE activation %d", x->se_act);
    MI355_REQUIRE((x->a_relu6 == 0 || x->a_relu6 == 1) && (x->has_res == 0 || x->has_res == 1),
                  "mbconv_block_ex: a_relu6=%d and has_res=%d are flags (0 / 1)", x->a_relu6, x->has_res);
    if (x->has_res) {
        MI355_REQUIRE(x->stride == 1, "mbconv_block_ex: a residual needs stride 1");
        MI355_REQUIRE(x->res_n >= 8 && x->res_n % 8 == 0 && x->res_n <= std::min(x->Cin, x->Cout),
                      "mbconv_block_ex: res_n=%d must be a multiple of 8 in 8 .. min(Cin, Cout) = %d", x->res_n, std::min(x->Cin, x->Cout));
    } else {
        MI355_REQUIRE(x->res_n == 0, "mbconv_block_ex: res_n=%d without a residual", x->res_n);
    }
    MI355_REQUIRE(x->norot >= 0 && x->norot <= 15, "mbconv_block_ex: norot=%d out of range 0..15", x->norot);
    for (const void* p : {x->X, x->We, (const void*)x->be, x->Wd, (const void*)x->bd, x->W1, (const void*)x->b1, x->W2, (const void*)x->b2,
                          x->Wp, (const void*)x->bp, (const void*)x->D, (const void*)x->Y})
        MI355_REQUIRE((uintptr_t)p % 16 == 0, "mbconv_block_ex: pointers must be 16-byte aligned");
    MI355_REQUIRE(mbconv_block_supported(x->H, x->W, x->Cin, x->mid, x->Cout, x->k, x->stride, x->rd, x->act_e, x->act_d),
                  "mbconv_block_ex: unsupported shape H=%d W=%d Cin=%d mid=%d Cout=%d k=%d stride=%d rd=%d act %d / %d", x->H, x->W, x->Cin,
                  x->mid, x->Cout, x->k, x->stride, x->rd, x->act_e, x->act_d);
    BlockArgs a = block_shape_args(x->H, x->W, x->Cin, x->mid, x->Cout, x->k, x->stride, x->rd, x->act_e, x->act_d);
    a.X = (const bf16_t*)x->X; a.We = (const bf16_t*)x->We; a.be = x->be; a.Wd = (const bf16_t*)x->Wd; a.bd = x->bd;
    a.W1 = (const bf16_t*)x->W1; a.b1 = x->b1; a.W2 = (const bf16_t*)x->W2; a.b2 = x->b2; a.Wp = (const bf16_t*)x->Wp; a.bp = x->bp;
    a.D = (bf16_t*)x->D; a.Y = (bf16_t*)x->Y;
    a.has_res = x->has_res; a.res_n = x->res_n; a.a_relu6 = x->a_relu6; a.se_act = x->se_act;
    a.norot = x->norot;             // variant = 0, stamps = null: no phase is skipped, nothing is timed
    return launch_mbconv_block(a, x->B, x->k, x->stride, (hipStream_t)stream, path);
}

int mi355_stem_ex(const mi355_stem_ex_args* x, int* path, void* stream) {
    if (path) *path = 0;
    MI355_REQUIRE(x, "stem_ex: null argument block");
    MI355_REQUIRE(x->w && x->bias && x->out, "stem_ex: null pointer (w, bias, out)");
    MI355_REQUIRE(!x->x != !x->images, "stem_ex: exactly one of x (fp32 form) and images (uint8 form) is given");
    MI355_REQUIRE(x->B >= 1 && x->B <= 65535 && x->H >= 1 && x->W >= 1 && x->H <= 16384 && x->W <= 16384,
                  "stem_ex: bad shape B=%d H=%d W=%d", x->B, x->H, x->W);
    MI355_REQUIRE(x->Cout >= 8 && x->Cout % 8 == 0 && x->Cout <= 256, "stem_ex: Cout=%d must be a multiple of 8 in 8..256", x->Cout);
    MI355_REQUIRE(x->act >= ACT_NONE && x->act <= ACT_SIGMOID, "stem_ex: unknown activation %d", x->act);
    for (const void* p : {(const void*)x->x, (const void*)x->w, (const void*)x->bias, (const void*)x->out})
        MI355_REQUIRE((uintptr_t)p % 16 == 0, "stem_ex: x, w, bias and out must be 16-byte aligned");
    const hipStream_t st = (hipStream_t)stream;
    if (x->x) {
        MI355_REQUIRE(!x->desc_host && !x->desc_dev && !x->conv_input_w,
                      "stem_ex: descriptors and conv_input belong to the uint8 form");
        return launch_stem(x->x, x->w, x->bias, (bf16_t*)x->out, x->B, x->H, x->W, x->Cout, x->act, st, path);
    }
    MI355_REQUIRE(x->mean && x->stdv, "stem_ex: null pointer (mean, stdv)");
    MI355_REQUIRE(x->fill >= 0 && x->fill <= 255, "stem_ex: fill %d is not a byte value", x->fill);
    for (int c = 0; c < 3; ++c) MI355_REQUIRE(x->stdv[c] != 0.f, "stem_ex: std[%d] is zero", c);
    MI355_REQUIRE((uintptr_t)x->conv_input_w % 4 == 0, "stem_ex: conv_input_w must be 4-byte aligned");
    MI355_REQUIRE(!x->desc_host == !x->desc_dev, "stem_ex: desc_host and desc_dev go together");
    if (x->desc_host) {
        if (int e = check_images(x->images, x->images_bytes, x->desc_host, x->desc_dev, x->B, "stem_ex")) return e;
        MI355_REQUIRE(x->H == x->W, "stem_ex: a ragged batch takes H == W == S, the common longer side (H=%d W=%d)", x->H, x->W);
        for (int b = 0; b < x->B; ++b) {
            const long long s = (long long)std::max(x->desc_host[(size_t)b * 3 + 1], x->desc_host[(size_t)b * 3 + 2]);
            MI355_REQUIRE(s == x->H, "stem_ex: image %d has longer side %lld, the batch's S is %d", b, s, x->H);
        }
    }
    return launch_stem_u8(x->images, x->H, x->W, x->fill, x->mean, x->stdv, x->conv_input_w, x->w, x->bias, (bf16_t*)x->out, x->B,
                          x->Cout, x->act, st, x->desc_dev, 0, path);
}

int mi355_head_gap_ex(const void* A, int lda, const void* W, int ldw, const float* bias, float* pooled, void* pooled_bf16, int ldp,
                      int B, int HW, int N, int K, int act, int* path, void* stream) {
    if (path) *path = 0;
    MI355_REQUIRE(A && W && bias && pooled, "head_gap_ex: null pointer");
    MI355_REQUIRE(B >= 1 && B <= 4 * 65535 && N >= 8, "head_gap_ex: bad shape B=%d N=%d", B, N);
    MI355_REQUIRE(head_gap_supported(HW, N, K, lda, ldw, act) && lda >= K,
                  "head_gap_ex: the kernel takes 1 <= HW <= 64, 32 <= K <= 512, lda a multiple of 8 and >= K, ldw a multiple of 32 "
                  "and >= K rounded up to 32, N a multiple of 8, act none or SiLU (HW=%d N=%d K=%d lda=%d ldw=%d act=%d)",
                  HW, N, K, lda, ldw, act);
    MI355_REQUIRE(ldp >= N && ldp % 2 == 0, "head_gap_ex: ldp=%d must be even and >= N=%d", ldp, N);
    for (const void* p : {A, W, (const void*)bias, (const void*)pooled, (const void*)pooled_bf16})
        MI355_REQUIRE((uintptr_t)p % 16 == 0, "head_gap_ex: pointers must be 16-byte aligned");
    return launch_head_gap((const bf16_t*)A, lda, (const bf16_t*)W, ldw, bias, pooled, (bf16_t*)pooled_bf16, ldp, B, HW, N, K, act,
                           (hipStream_t)stream, path);
}

int mi355_gap(const void* in, int B, int HW, int C, float* pooled, void* pooled_bf16, void* stream) {
    MI355_REQUIRE(in && pooled, "gap: null pointer");
    MI355_REQUIRE(B >= 1 && HW >= 1 && C >= 8, "gap: bad shape B=%d HW=%d C=%d", B, HW, C);
    MI355_REQUIRE(C % 8 == 0, "gap: C=%d must be a multiple of 8", C);
    MI355_REQUIRE((long)B * (C / 8) < (1l << 31), "gap: B=%d x C=%d too large", B, C);
    for (const void* p : {in, (const void*)pooled, (const void*)pooled_bf16})
        MI355_REQUIRE((uintptr_t)p % 16 == 0, "gap: pointers must be 16-byte aligned");
    return launch_gap((const bf16_t*)in, pooled, (bf16_t*)pooled_bf16, B, HW, C, (hipStream_t)stream);
}

// the layout kernels' grid is (HW / 32, C / 32, B)
static int layout_args_ok(const char* who, const void* in, const void* out, int B, int HW, int C, int Cvalid, int in_align) {
    MI355_REQUIRE(in && out, "%s: null pointer", who);
    MI355_REQUIRE(B >= 1 && B <= 65535 && HW >= 1 && C >= 1 && C <= 32 * 65535, "%s: bad shape B=%d HW=%d C=%d", who, B, HW, C);
    MI355_REQUIRE(Cvalid >= 1 && Cvalid <= C, "%s: Cvalid=%d outside 1..C=%d", who, Cvalid, C);
    MI355_REQUIRE((uintptr_t)in % in_align == 0 && (uintptr_t)out % (6 - in_align) == 0,
                  "%s: pointers must be aligned to their element size", who);
    return OK;
}

int mi355_nhwc_to_nchw(const void* in, float* out, int B, int HW, int C, int Cvalid, void* stream) {
    if (int e = layout_args_ok("nhwc_to_nchw", in, out, B, HW, C, Cvalid, 2)) return e;
    return launch_nhwc_to_nchw_f32((const bf16_t*)in, out, B, HW, C, Cvalid, (hipStream_t)stream);
}

int mi355_nchw_to_nhwc(const float* in, void* out, int B, int HW, int C, int Cvalid, void* stream) {
    if (int e = layout_args_ok("nchw_to_nhwc", in, out, B, HW, C, Cvalid, 4)) return e;
    return launch_nchw_f32_to_nhwc_bf16(in, (bf16_t*)out, B, HW, Cvalid, C, (hipStream_t)stream);
}

int mi355_pool_linear(const float* fm, int B, int C, int HW, const float* weight, const float* bias, int N, float* out,
                      float* pooled_out, void* stream) {
    MI355_REQUIRE(fm && (out || pooled_out), "pool_linear: null pointer");
    MI355_REQUIRE(B >= 1 && C >= 1 && HW >= 1, "pool_linear: bad shape B=%d C=%d HW=%d", B, C, HW);
    MI355_REQUIRE(!weight || (N >= 1 && out), "pool_linear: a weight needs N >= 1 and an output");
    return launch_pool_linear(fm, weight, bias, out, pooled_out, B, C, HW, weight ? N : 0, (hipStream_t)stream);
}

int mi355_square_pad_normalize(const unsigned char* img, int h, int w, int fill, const float* mean, const float* stdv,
                               float* out, void* stream) {
    MI355_REQUIRE(img && mean && stdv && out, "square_pad_normalize: null pointer");
    MI355_REQUIRE(h >= 1 && w >= 1 && h <= 16384 && w <= 16384, "square_pad_normalize: bad image size %dx%d", h, w);
    MI355_REQUIRE(fill >= 0 && fill <= 255, "square_pad_normalize: fill must be a byte value");
    for (int c = 0; c < 3; ++c) MI355_REQUIRE(stdv[c] != 0.f, "square_pad_normalize: std[%d] is zero", c);
    return launch_square_pad_normalize(img, h, w, fill, mean, stdv, out, (hipStream_t)stream);
}

int mi355_conv_input_silu(const float* x, const float* w, int B, int H, int W, float* out, void* stream) {
    MI355_REQUIRE(x && w && out, "conv_input_silu: null pointer");
    MI355_REQUIRE(B >= 1 && H >= 1 && W >= 1, "conv_input_silu: bad shape");
    return launch_conv_input_silu(x, w, B, H, W, out, (hipStream_t)stream);
}

}  // extern "C"
