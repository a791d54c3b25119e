// Training-side pre-processing and score post-processing that sit either side of the hot path.
//
//   mi355_resize_bilinear_u8   transforms.Resize((h, w)) of train/train.py:48-50 on a PIL image ==
//                              Pillow's two-pass antialiased BILINEAR resample (Resample.c, 8-bit path): per-axis
//                              triangle-filter coefficients in double, fixed point 2^22, uint8 between the passes.
//                              The coefficient tables are built on the host exactly as Pillow builds them and cached on
//                              the device per (device, in, out); the passes are integer MACs => bit-exact with Pillow.
//   mi355_resize_batch_u8      the same resample for a ragged batch (images of any sizes, packed in one buffer and described
//                              by {byte offset, h, w}) into one uniform uint8 batch: one horizontal and one vertical launch
//                              for the whole batch, optionally on each image's virtual SquarePad(fill) square.
//   mi355_score_boost          utils/score_booster.py:1-37 over a whole score tensor.
#include "common.h"
#include "ops.h"
#include "../../include/mi355_retrieval.h"
#include <algorithm>
#include <map>
#include <math.h>
#include <mutex>
#include <string.h>
#include <tuple>
#include <vector>

namespace mi355 {

constexpr int RS_PRECISION_BITS = 32 - 8 - 2;

struct ResizeCoeffs {
    int ksize = 0;
    std::vector<int> host;   // [out][2 + ksize]: first source index, tap count, taps (kept alive for the async upload)
    int* dev = nullptr;
};

// Pillow's source window of output xx: [xmin, xend) of the input (precompute_coeffs, bilinear support 1.0, box = (0, in)).
struct BoxGeom {
    double scale, filterscale, support;
    BoxGeom(int in_size, int out_size) {
        scale = (double)((float)in_size - 0.0f) / out_size;
        filterscale = scale < 1.0 ? 1.0 : scale;
        support = 1.0 * filterscale;
    }
    void span(int in_size, int xx, int* xmin, int* xend) const {
        const double center = 0.0 + (xx + 0.5) * scale;
        int lo = (int)(center - support + 0.5);
        if (lo < 0) lo = 0;
        int hi = (int)(center + support + 0.5);
        if (hi > in_size) hi = in_size;
        *xmin = lo;
        *xend = hi;
    }
};

// Pillow precompute_coeffs + normalize_coeffs_8bpc for the bilinear (triangle, support 1.0) filter, box = (0, in).
static void build_coeffs(int in_size, int out_size, ResizeCoeffs& rc) {
    const BoxGeom g(in_size, out_size);
    const double scale = g.scale, filterscale = g.filterscale, support = g.support;
    const int ksize = (int)ceil(support) * 2 + 1;
    rc.ksize = ksize;
    rc.host.assign((size_t)out_size * (2 + ksize), 0);
    std::vector<double> k(ksize);
    const double ss = 1.0 / filterscale;
    for (int xx = 0; xx < out_size; ++xx) {
        const double center = 0.0 + (xx + 0.5) * scale;
        double ww = 0.0;
        int xmin, xmax;
        g.span(in_size, xx, &xmin, &xmax);
        xmax -= xmin;
        int x = 0;
        for (; x < xmax; ++x) {
            double a = (x + xmin - center + 0.5) * ss;
            if (a < 0.0) a = -a;
            const double w = a < 1.0 ? 1.0 - a : 0.0;
            k[x] = w;
            ww += w;
        }
        for (x = 0; x < xmax; ++x)
            if (ww != 0.0) k[x] /= ww;
        for (; x < ksize; ++x) k[x] = 0.0;
        int* row = rc.host.data() + (size_t)xx * (2 + ksize);
        row[0] = xmin;
        row[1] = xmax;
        for (x = 0; x < ksize; ++x)
            row[2 + x] = k[x] < 0 ? (int)(-0.5 + k[x] * (1 << RS_PRECISION_BITS)) : (int)(0.5 + k[x] * (1 << RS_PRECISION_BITS));
    }
}

static std::mutex g_rs_mu;
static std::map<std::tuple<int, int, int>, ResizeCoeffs> g_rs_cache;

static int get_coeffs(int in_size, int out_size, hipStream_t st, const ResizeCoeffs** out) {
    int dev = 0;
    MI355_CHECK_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(g_rs_mu);
    auto key = std::make_tuple(dev, in_size, out_size);
    auto it = g_rs_cache.find(key);
    if (it == g_rs_cache.end()) {
        ResizeCoeffs rc;
        build_coeffs(in_size, out_size, rc);
        MI355_CHECK_HIP(hipMalloc((void**)&rc.dev, rc.host.size() * sizeof(int)));
        it = g_rs_cache.emplace(key, std::move(rc)).first;
        MI355_CHECK_HIP(hipMemcpyAsync(it->second.dev, it->second.host.data(), it->second.host.size() * sizeof(int),
                                       hipMemcpyHostToDevice, st));
        // one-time upload: finish it before the table is published, so that a later caller on ANOTHER stream never
        // reads a table whose copy is still queued behind the first caller's stream
        MI355_CHECK_HIP(hipStreamSynchronize(st));
    }
    *out = &it->second;
    return OK;
}

// Tables for every (in, out) pair of `sizes`, in order.  The pairs this device has not seen yet are built together and uploaded
// with ONE allocation, ONE copy and ONE synchronise (a batch of photos brings many first-seen sizes at once).
static int get_coeffs_many(const std::vector<std::pair<int, int>>& sizes, hipStream_t st, std::vector<const ResizeCoeffs*>& out) {
    int dev = 0;
    MI355_CHECK_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(g_rs_mu);
    std::map<std::tuple<int, int, int>, ResizeCoeffs> fresh;
    size_t total = 0;
    for (const auto& io : sizes) {
        const auto key = std::make_tuple(dev, io.first, io.second);
        if (g_rs_cache.count(key) || fresh.count(key)) continue;
        ResizeCoeffs& rc = fresh[key];
        build_coeffs(io.first, io.second, rc);
        total += rc.host.size();
    }
    if (!fresh.empty()) {
        std::vector<int> host;
        host.reserve(total);
        for (auto& kv : fresh) host.insert(host.end(), kv.second.host.begin(), kv.second.host.end());
        int* block = nullptr;
        MI355_CHECK_HIP(hipMalloc((void**)&block, total * sizeof(int)));
        MI355_CHECK_HIP(hipMemcpyAsync(block, host.data(), total * sizeof(int), hipMemcpyHostToDevice, st));
        // as in get_coeffs: the tables are complete before any stream can find them in the cache
        MI355_CHECK_HIP(hipStreamSynchronize(st));
        size_t off = 0;
        for (auto& kv : fresh) {
            kv.second.dev = block + off;
            off += kv.second.host.size();
            g_rs_cache.emplace(kv.first, std::move(kv.second));
        }
    }
    out.clear();
    for (const auto& io : sizes) out.push_back(&g_rs_cache.at(std::make_tuple(dev, io.first, io.second)));
    return OK;
}

// One pass along x: out[r][ox][c] = clip8((2^21 + sum_i in[r0 + r][xmin + i][c] * k_i) >> 22).  thread = (row, ox).
__global__ __launch_bounds__(256) void k_resize_h(const unsigned char* __restrict__ in, int w, int row0, int rows,
                                                  unsigned char* __restrict__ out, int out_w,
                                                  const int* __restrict__ coef, int ksize) {
    const int ox = blockIdx.x * 64 + (threadIdx.x & 63);
    const int r = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (ox >= out_w || r >= rows) return;
    const int* row = coef + (size_t)ox * (2 + ksize);
    const int xmin = row[0], n = row[1];
    int a0 = 1 << (RS_PRECISION_BITS - 1), a1 = a0, a2 = a0;
    const unsigned char* p = in + ((size_t)(row0 + r) * w + xmin) * 3;
    for (int i = 0; i < n; ++i) {
        const int k = row[2 + i];
        a0 += (int)p[i * 3 + 0] * k;
        a1 += (int)p[i * 3 + 1] * k;
        a2 += (int)p[i * 3 + 2] * k;
    }
    unsigned char* o = out + ((size_t)r * out_w + ox) * 3;
    o[0] = (unsigned char)min(max(a0 >> RS_PRECISION_BITS, 0), 255);
    o[1] = (unsigned char)min(max(a1 >> RS_PRECISION_BITS, 0), 255);
    o[2] = (unsigned char)min(max(a2 >> RS_PRECISION_BITS, 0), 255);
}

// One pass along y over an image of `w` pixels per row: thread = (oy, byte of the row), coalesced along the row.
__global__ __launch_bounds__(256) void k_resize_v(const unsigned char* __restrict__ in, int w, int row_shift,
                                                  unsigned char* __restrict__ out, int out_h,
                                                  const int* __restrict__ coef, int ksize) {
    const int xb = blockIdx.x * 256 + threadIdx.x;   // byte within the row (3 * w of them)
    const int oy = blockIdx.y;
    if (xb >= 3 * w || oy >= out_h) return;
    const int* row = coef + (size_t)oy * (2 + ksize);
    const int ymin = row[0] - row_shift, n = row[1];
    int acc = 1 << (RS_PRECISION_BITS - 1);
    for (int i = 0; i < n; ++i) acc += (int)in[(size_t)(ymin + i) * 3 * w + xb] * row[2 + i];
    out[(size_t)oy * 3 * w + xb] = (unsigned char)min(max(acc >> RS_PRECISION_BITS, 0), 255);
}

// ---- ragged batches ---------------------------------------------------------------------------------------------------
// Per image: its two tables and where its horizontal-pass rows live.  The geometry (byte offset, h, w) is the caller's
// device descriptor desc[b] = {offset, h, w}; in pad mode the image is resampled as the centre of its S x S SquarePad square,
// S = max(h, w), whose border reads `fill` (no padded copy exists).
struct RsPlan {
    const int* hc;      // source width (w, or S) -> out_w: out_w rows of 2 + hk ints
    const int* vc;      // source height (h, or S) -> out_h: out_h rows of 2 + vk ints
    int64_t tmp;        // byte offset of the image's rows [rows][pitch] in the temporary (pitch = 3 * out_w rounded up to 4)
    int hk, vk;
    int first, rows;    // source rows [first, first + rows) = every row the vertical pass reads
};
constexpr int RSB_ROWS = 4;   // temporary rows per horizontal-pass workgroup (x 64 output columns)

// Horizontal pass over the whole batch: blockIdx.x walks the images' row blocks (rb0[i] = first block of image i, a host prefix
// sum, rb0[B] = total), blockIdx.y the output columns.  Same integer MAC, rounding and clip as k_resize_h; a source pixel outside
// the image (pad mode only) is `fill` and goes through the same MAC - the taps need not sum to 2^22, so a border pixel is not fill.
__global__ __launch_bounds__(256) void k_resize_h_batch(const unsigned char* __restrict__ px, const int64_t* __restrict__ desc,
                                                        const RsPlan* __restrict__ plan, const int* __restrict__ rb0, int B,
                                                        int pad, int fill, unsigned char* __restrict__ tmp, int out_w,
                                                        int pitch) {
    const int blk = blockIdx.x;
    int lo = 0, hi = B - 1;   // the last image whose first block is <= blk (every image has at least one block)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (rb0[mid] <= blk) lo = mid;
        else hi = mid - 1;
    }
    const RsPlan t = plan[lo];
    const int r = (blk - rb0[lo]) * RSB_ROWS + (threadIdx.x >> 6);
    const int ox = blockIdx.y * 64 + (threadIdx.x & 63);
    if (ox >= out_w || r >= t.rows) return;
    const int64_t* d = desc + (size_t)lo * 3;
    const int h = (int)d[1], w = (int)d[2], S = max(h, w);
    const int hp = pad ? (S - w) / 2 : 0, vp = pad ? (S - h) / 2 : 0;
    const int iy = t.first + r - vp;
    const bool row_in = iy >= 0 && iy < h;
    const unsigned char* p = px + d[0] + (size_t)(row_in ? iy : 0) * w * 3;
    const int* row = t.hc + (size_t)ox * (2 + t.hk);
    const int x0 = row[0] - hp, n = row[1];
    int a0 = 1 << (RS_PRECISION_BITS - 1), a1 = a0, a2 = a0;
    // unrolled with a clamped (always valid) address, so the loads of several taps are in flight together: one load after
    // another made both passes latency-bound
#pragma unroll 4
    for (int i = 0; i < n; ++i) {
        const int k = row[2 + i];
        const int ix = x0 + i;
        const bool in = row_in && ix >= 0 && ix < w;
        const unsigned char* q = p + (size_t)min(max(ix, 0), w - 1) * 3;
        const int v0 = q[0], v1 = q[1], v2 = q[2];
        a0 += (in ? v0 : fill) * k;
        a1 += (in ? v1 : fill) * k;
        a2 += (in ? v2 : fill) * k;
    }
    unsigned char* o = tmp + t.tmp + (size_t)r * pitch + (size_t)ox * 3;
    o[0] = (unsigned char)min(max(a0 >> RS_PRECISION_BITS, 0), 255);
    o[1] = (unsigned char)min(max(a1 >> RS_PRECISION_BITS, 0), 255);
    o[2] = (unsigned char)min(max(a2 >> RS_PRECISION_BITS, 0), 255);
}

// Vertical pass into the uniform batch out[B][out_h][out_w][3]: blockIdx.x = (image, oy), thread = 4 bytes of the row (one dword
// of the temporary, whose row pitch is a multiple of 4; the pitch padding is read but never stored), same MAC as k_resize_v.
__global__ __launch_bounds__(256) void k_resize_v_batch(const RsPlan* __restrict__ plan, const unsigned char* __restrict__ tmp,
                                                        unsigned char* __restrict__ out, int out_h, int out_w, int pitch) {
    const int b = blockIdx.x / out_h, oy = blockIdx.x - b * out_h;
    const int xb = (blockIdx.y * 256 + threadIdx.x) * 4;
    const int row_bytes = 3 * out_w;
    if (xb >= row_bytes) return;
    const RsPlan t = plan[b];
    const int* row = t.vc + (size_t)oy * (2 + t.vk);
    const int ymin = row[0] - t.first, n = row[1];
    const unsigned* src = reinterpret_cast<const unsigned*>(tmp + t.tmp + xb);
    const int pw = pitch >> 2;
    int a0 = 1 << (RS_PRECISION_BITS - 1), a1 = a0, a2 = a0, a3 = a0;
#pragma unroll 4
    for (int i = 0; i < n; ++i) {
        const unsigned v = src[(size_t)(ymin + i) * pw];
        const int k = row[2 + i];
        a0 += (int)(v & 255u) * k;
        a1 += (int)((v >> 8) & 255u) * k;
        a2 += (int)((v >> 16) & 255u) * k;
        a3 += (int)(v >> 24) * k;
    }
    const unsigned o0 = min(max(a0 >> RS_PRECISION_BITS, 0), 255), o1 = min(max(a1 >> RS_PRECISION_BITS, 0), 255),
                   o2 = min(max(a2 >> RS_PRECISION_BITS, 0), 255), o3 = min(max(a3 >> RS_PRECISION_BITS, 0), 255);
    unsigned char* o = out + ((size_t)b * out_h + oy) * row_bytes + xb;
    if ((row_bytes & 3) == 0) {
        *reinterpret_cast<unsigned*>(o) = o0 | (o1 << 8) | (o2 << 16) | (o3 << 24);
    } else {     // rows are not dword aligned: byte stores, and the row's last dword may be partial
        o[0] = (unsigned char)o0;
        if (xb + 1 < row_bytes) o[1] = (unsigned char)o1;
        if (xb + 2 < row_bytes) o[2] = (unsigned char)o2;
        if (xb + 3 < row_bytes) o[3] = (unsigned char)o3;
    }
}

// Pinned host staging for the per-call plan.  A buffer is handed out again only once the copy that last read it has run (its
// event), so a second call never overwrites a plan that is still queued behind the first one.
struct Staging {
    int dev;
    void* host;
    size_t cap;
    hipEvent_t done;
};
static std::mutex g_stage_mu;
static std::vector<Staging> g_stage;

static int upload_async(void* dst, const void* src, size_t bytes, hipStream_t st) {
    int dev = 0;
    MI355_CHECK_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(g_stage_mu);
    Staging* s = nullptr;
    for (auto& e : g_stage)
        if (e.dev == dev && e.cap >= bytes && hipEventQuery(e.done) == hipSuccess) { s = &e; break; }
    if (!s) {
        Staging n{dev, nullptr, std::max(bytes, (size_t)1 << 16), nullptr};
        MI355_CHECK_HIP(hipHostMalloc(&n.host, n.cap, hipHostMallocDefault));
        MI355_CHECK_HIP(hipEventCreateWithFlags(&n.done, hipEventDisableTiming));
        g_stage.push_back(n);
        s = &g_stage.back();
    }
    memcpy(s->host, src, bytes);
    MI355_CHECK_HIP(hipMemcpyAsync(dst, s->host, bytes, hipMemcpyHostToDevice, st));
    MI355_CHECK_HIP(hipEventRecord(s->done, st));
    return OK;
}

// Source extent of image b as the resample sees it: the image itself, or its S x S square in pad mode.
static void rs_source(const int64_t* desc, int b, bool pad, int* sh, int* sw) {
    const int h = (int)desc[(size_t)b * 3 + 1], w = (int)desc[(size_t)b * 3 + 2];
    *sh = pad ? std::max(h, w) : h;
    *sw = pad ? std::max(h, w) : w;
}

static int rs_pitch(int out_w) { return (int)align_up((size_t)3 * out_w, 4); }

static size_t rs_plan_bytes(int B) { return align_up((size_t)B * sizeof(RsPlan) + (size_t)(B + 1) * sizeof(int), 256); }

// Host-only layout of the temporary: rows of every image (first / rows per image) and the total workspace.
static size_t rs_layout(const int64_t* desc, int B, int out_h, int out_w, bool pad, std::vector<int>* first, std::vector<int>* rows) {
    size_t tmp = 0;
    for (int b = 0; b < B; ++b) {
        int sh, sw;
        rs_source(desc, b, pad, &sh, &sw);
        const BoxGeom g(sh, out_h);
        int f, unused, e;
        g.span(sh, 0, &f, &unused);            // ybox_first .. ybox_last of Pillow's ImagingResample
        g.span(sh, out_h - 1, &unused, &e);
        if (first) { first->push_back(f); rows->push_back(e - f); }
        tmp += (size_t)(e - f) * rs_pitch(out_w);
    }
    return rs_plan_bytes(B) + align_up(tmp, 256);
}

__global__ __launch_bounds__(256) void k_score_boost(const float* __restrict__ s, float* __restrict__ out, long n,
                                                     float eps, float alpha, float threshold, int mode) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float v = s[i];
    // mode 0: by threshold; 1: "for_pos"; 2: "for_neg" (utils/score_booster.py:17-20, 33-36); same fp32 op order
    const bool pos = mode == 1 || (mode == 0 && v >= threshold);
    const bool neg = mode == 2 || (mode == 0 && v < threshold);
    float r = v;                                     // NaN under mode 0 matches neither branch (python returns None)
    if (pos) r = (v + eps) / (eps + alpha);
    else if (neg) r = fabsf((v + (alpha / eps)) / (2.0f * eps));
    out[i] = r;
}

int check_images(const unsigned char* pixels, int64_t pixels_bytes, const int64_t* desc_host, const int64_t* desc_dev, int B,
                 const char* who) {
    MI355_REQUIRE(pixels && desc_host && desc_dev, "%s: null pixels / descriptor pointer", who);
    MI355_REQUIRE(B >= 1, "%s: B=%d must be >= 1", who, B);
    for (int b = 0; b < B; ++b) {
        const int64_t off = desc_host[(size_t)b * 3], h = desc_host[(size_t)b * 3 + 1], w = desc_host[(size_t)b * 3 + 2];
        MI355_REQUIRE(h >= 1 && w >= 1 && h <= 16384 && w <= 16384, "%s: image %d has a bad size %lldx%lld", who, b,
                      (long long)h, (long long)w);
        MI355_REQUIRE(off >= 0 && off <= pixels_bytes - h * w * 3, "%s: image %d (%lld bytes at offset %lld) is outside the "
                      "%lld-byte pixel buffer", who, b, (long long)(h * w * 3), (long long)off, (long long)pixels_bytes);
    }
    return OK;
}

size_t resize_batch_workspace(const int64_t* desc_host, int B, int out_h, int out_w, bool pad) {
    if (!desc_host || B < 1 || out_h < 1 || out_w < 1 || out_h > 16384 || out_w > 16384) return 0;
    for (int b = 0; b < B; ++b) {
        const int64_t h = desc_host[(size_t)b * 3 + 1], w = desc_host[(size_t)b * 3 + 2];
        if (h < 1 || w < 1 || h > 16384 || w > 16384) return 0;
    }
    return rs_layout(desc_host, B, out_h, out_w, pad, nullptr, nullptr);
}

int resize_batch(const unsigned char* pixels, int64_t pixels_bytes, const int64_t* desc_host, const int64_t* desc_dev, int B,
                 int out_h, int out_w, bool pad, int fill, unsigned char* out, void* workspace, size_t workspace_bytes,
                 hipStream_t st) {
    if (int e = check_images(pixels, pixels_bytes, desc_host, desc_dev, B, "resize_batch")) return e;
    MI355_REQUIRE(out, "resize_batch: null output pointer");
    MI355_REQUIRE(out_h >= 1 && out_w >= 1 && out_h <= 16384 && out_w <= 16384, "resize_batch: bad output size %dx%d", out_h, out_w);
    MI355_REQUIRE(fill >= 0 && fill <= 255, "resize_batch: fill %d is not a byte value", fill);
    MI355_REQUIRE((int64_t)B * out_h <= INT32_MAX, "resize_batch: B * out_h = %lld is too large", (long long)B * out_h);
    std::vector<int> first, rows;
    const size_t need = rs_layout(desc_host, B, out_h, out_w, pad, &first, &rows);
    MI355_REQUIRE(workspace && workspace_bytes >= need, "resize_batch: workspace of %zu bytes < %zu "
                  "(mi355_resize_batch_workspace_bytes)", workspace_bytes, need);
    std::vector<int> host(((size_t)B * sizeof(RsPlan) + (size_t)(B + 1) * sizeof(int) + sizeof(int) - 1) / sizeof(int));
    RsPlan* plan = reinterpret_cast<RsPlan*>(host.data());
    int* rb0 = reinterpret_cast<int*>(plan + B);
    int64_t blocks = 0, tmp = 0;
    for (int b = 0; b < B; ++b) {
        rb0[b] = (int)blocks;
        blocks += cdiv(rows[b], RSB_ROWS);
        MI355_REQUIRE(blocks <= INT32_MAX, "resize_batch: too many source rows");
        plan[b].tmp = tmp;
        plan[b].first = first[b];
        plan[b].rows = rows[b];
        tmp += (int64_t)rows[b] * rs_pitch(out_w);
    }
    rb0[B] = (int)blocks;
    std::vector<std::pair<int, int>> sizes;
    sizes.reserve(2 * (size_t)B);
    for (int b = 0; b < B; ++b) {
        int sh, sw;
        rs_source(desc_host, b, pad, &sh, &sw);
        sizes.emplace_back(sw, out_w);
        sizes.emplace_back(sh, out_h);
    }
    std::vector<const ResizeCoeffs*> tabs;
    if (int e = get_coeffs_many(sizes, st, tabs)) return e;
    for (int b = 0; b < B; ++b) {
        plan[b].hc = tabs[2 * b]->dev;
        plan[b].hk = tabs[2 * b]->ksize;
        plan[b].vc = tabs[2 * b + 1]->dev;
        plan[b].vk = tabs[2 * b + 1]->ksize;
    }
    char* ws = (char*)workspace;
    const RsPlan* dplan = reinterpret_cast<const RsPlan*>(ws);
    const int* drb0 = reinterpret_cast<const int*>(dplan + B);
    unsigned char* dtmp = (unsigned char*)ws + rs_plan_bytes(B);
    if (int e = upload_async(ws, host.data(), (size_t)B * sizeof(RsPlan) + (size_t)(B + 1) * sizeof(int), st)) return e;
    hipLaunchKernelGGL(k_resize_h_batch, dim3((unsigned)blocks, cdiv(out_w, 64)), dim3(256), 0, st, pixels, desc_dev, dplan, drb0,
                       B, (int)pad, fill, dtmp, out_w, rs_pitch(out_w));
    MI355_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_resize_v_batch, dim3((unsigned)(B * out_h), cdiv(3 * out_w, 1024)), dim3(256), 0, st, dplan,
                       (const unsigned char*)dtmp, out, out_h, out_w, rs_pitch(out_w));
    MI355_LAUNCH_CHECK();
    return OK;
}

}  // namespace mi355

using namespace mi355;

extern "C" {

int mi355_resize_bilinear_u8(const unsigned char* img, int h, int w, unsigned char* out, int out_h, int out_w,
                             unsigned char* tmp, void* stream) {
    MI355_REQUIRE(img && out, "resize: null pointer");
    MI355_REQUIRE(h >= 1 && w >= 1 && h <= 16384 && w <= 16384, "resize: bad input size %dx%d", h, w);
    MI355_REQUIRE(out_h >= 1 && out_w >= 1 && out_h <= 16384 && out_w <= 16384, "resize: bad output size %dx%d", out_h, out_w);
    hipStream_t st = (hipStream_t)stream;
    const bool need_h = w != out_w, need_v = h != out_h;
    if (!need_h && !need_v) {   // PIL returns a copy
        MI355_CHECK_HIP(hipMemcpyAsync(out, img, (size_t)h * w * 3, hipMemcpyDeviceToDevice, st));
        return OK;
    }
    const ResizeCoeffs *ch = nullptr, *cv = nullptr;
    if (need_h) { const int e = get_coeffs(w, out_w, st, &ch); if (e) return e; }
    if (need_v) { const int e = get_coeffs(h, out_h, st, &cv); if (e) return e; }
    int first = 0, last = h;
    if (need_v) {   // the horizontal pass only produces the rows the vertical pass reads (ybox_first .. ybox_last)
        const int stride = 2 + cv->ksize;
        first = cv->host[0];
        last = cv->host[(size_t)(out_h - 1) * stride] + cv->host[(size_t)(out_h - 1) * stride + 1];
    }
    const unsigned char* vsrc = img;
    int shift = 0;
    if (need_h) {
        unsigned char* hdst = need_v ? tmp : out;
        MI355_REQUIRE(hdst != nullptr, "resize: tmp (h * out_w * 3 bytes) is required when both sides change");
        const int rows = last - first;
        hipLaunchKernelGGL(k_resize_h, dim3(cdiv(out_w, 64), cdiv(rows, 4)), dim3(256), 0, st, img, w, first, rows, hdst,
                           out_w, ch->dev, ch->ksize);
        MI355_LAUNCH_CHECK();
        vsrc = hdst;
        shift = first;
    }
    if (need_v) {
        hipLaunchKernelGGL(k_resize_v, dim3(cdiv(3 * out_w, 256), out_h), dim3(256), 0, st, vsrc, out_w, shift, out, out_h,
                           cv->dev, cv->ksize);
        MI355_LAUNCH_CHECK();
    }
    return OK;
}

size_t mi355_resize_batch_workspace_bytes(const int64_t* desc_host, int B, int out_h, int out_w, int pad) {
    return resize_batch_workspace(desc_host, B, out_h, out_w, pad != 0);
}

int mi355_resize_batch_u8(const unsigned char* pixels, int64_t pixels_bytes, const int64_t* desc_host, const int64_t* desc_dev, int B,
                          int out_h, int out_w, int pad, int fill, unsigned char* out, void* workspace, size_t workspace_bytes,
                          void* stream) {
    return resize_batch(pixels, pixels_bytes, desc_host, desc_dev, B, out_h, out_w, pad != 0, fill, out, workspace,
                        workspace_bytes, (hipStream_t)stream);
}

int mi355_score_boost(const float* scores, int64_t n, float eps, float alpha, float threshold, int mode, float* out,
                      void* stream) {
    MI355_REQUIRE(n >= 0, "score_boost: n=%lld", (long long)n);
    MI355_REQUIRE(mode >= 0 && mode <= 2, "score_boost: mode %d (0 = threshold, 1 = for_pos, 2 = for_neg)", mode);
    if (n == 0) return OK;
    MI355_REQUIRE(scores && out, "score_boost: null pointer");
    hipLaunchKernelGGL(k_score_boost, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, scores, out, (long)n,
                       eps, alpha, threshold, mode);
    MI355_LAUNCH_CHECK();
    return OK;
}

}  // extern "C"
