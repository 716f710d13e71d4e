// prk_span_pass.hip — the whole-object pass of a flush (flush_spans): draws of
// objects of more than one triangle, caller edges, edge lists, spans and the
// record / span handles.  SpanPass holds what its phases share: plan (host
// only), upload, edges, sizes, classify (the large objects' walks: one
// walk-class rule, slot_class), chunked, walk, bin_shade.  The kernels are
// prk_spans.hip's, through prk_launch.h; prk_flush (prk_flush.hip) calls
// flush_spans for every maximal run of such draws.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "prk_ctx.h"

using prk::EdgeIn;
using prk::ListSrc;
using prk::MaxactLayout;
using prk::ObjDesc;
using prk::ObjEdge;
using prk::ObjRun;
using prk::ObjSeg;
using prk::PairRaw;
using prk::PrObj;
using prk::PrRow;
using prk::PrepSeg;
using prk::ScSpanRec;
using prk::SpanPos;
using prk::SpanRec;
using prk::SpanRecG;
using prk::kAdvWgCaps;
using prk::kPrepEdges;
using prk::kWaveListArrays;

namespace {

// The switches a span pass (flush_spans) obeys, read from the environment at
// the start of every pass: tests set and unset them between the flushes of
// one process.
struct SpanSwitches {
    // PRK_OBJ_LOCAL_SORT=0: one radix sort of the padded keys even when no
    // object has more than 64 edges (else per object, k_obj_sort_local)
    bool local_sort = !off("PRK_OBJ_LOCAL_SORT");
    // PRK_OBJ_SEGMENTS=0: the small objects a thread per object, not a thread
    // per stretch of rows with a non-empty list (k_obj_seg)
    bool segments = !off("PRK_OBJ_SEGMENTS");
    // PRK_OBJ_HUGE_EDGES=n (tests): objects of n edges or more, not of 2^18,
    // are sized by many workgroups each (k_maxact_huge_*)
    uint32_t huge_edges = 1u << 18;
    // PRK_OBJ_BIG=0: an object past the slot classes is always walked by one
    // wave (k_obj_walk_wave), never by the huge-object walk
    bool big = !off("PRK_OBJ_BIG");
    // PRK_OBJ_LDSWALK=0: the huge-object walk never in its LDS form (k_obj_walk_lds)
    bool ldswalk = !off("PRK_OBJ_LDSWALK");
    // PRK_OBJ_BIG_MIN=n (tests): objects of more than n active edges skip the
    // walk groups' slot classes (the chunked walk's groups do not look at it)
    int64_t big_min = INT64_MAX;
    // PRK_OBJ_ROWS=0: no chunked walk; every large object takes the workgroup walk alone
    bool rows = !off("PRK_OBJ_ROWS");
    // PRK_OBJ_CHUNK_WARMUP=0 (tests: every fix-up path): the chunked walk without its warm-up
    bool chunk_warmup = !off("PRK_OBJ_CHUNK_WARMUP");
    // PRK_POS_MEMSET=1: the span slots are marked unused by a memset even in a
    // pass without large objects (whose walks mark their own)
    bool pos_memset = false;
    // PRK_PR_DEBUG: a line about the pass's chunked walk on stderr
    bool pr_debug = std::getenv("PRK_PR_DEBUG") != nullptr;
    SpanSwitches() {
        if (const char *env = std::getenv("PRK_OBJ_HUGE_EDGES")) huge_edges = (uint32_t)std::max(1l, std::atol(env));
        if (const char *env = std::getenv("PRK_OBJ_BIG_MIN")) big_min = std::atoll(env);
        const char *env = std::getenv("PRK_POS_MEMSET");
        pos_memset = env && env[0] == '1';
    }
    static bool off(const char *name) {
        const char *env = std::getenv(name);
        return env && env[0] == '0';
    }
};

// The slot class of a large object whose list holds `most` entries at the
// most: the smallest of the slot walk's LDS capacities (kAdvWgCaps) that holds
// them and that the device grants (lcap), or 0 for none.
uint32_t slot_class(int32_t most, uint32_t lcap) {
    if (most < 0) return 0;
    for (const uint32_t cap : kAdvWgCaps)
        if (cap <= lcap && (uint32_t)most <= cap) return cap;
    return 0;
}

// The classification block of a pass with n large objects (SpanScratch
// h_cls, d_cls), one layout for the host's pinned copy and the device's:
// (most, rows, entries) as k_obj_maxact writes them (MaxactLayout), then the
// walk groups' objects, pool offsets and list capacities, the chunked walk's
// table (PrObj) and its objects by group, and the huge walk's (rows, entries)
// per object in walk-group order.
struct ClsView {
    int32_t *most, *rows, *ents;
    uint32_t *big;
    unsigned long long *off;
    uint32_t *cap;
    PrObj *pr;
    uint32_t *grp, *meta;
};
struct ClsLayout {
    size_t n, big, off, cap, pr, grp, meta, end;
    explicit ClsLayout(uint32_t nbig = 0) : n(nbig) {
        big = MaxactLayout{n}.bytes();
        off = (big + 4 * n + 7) & ~(size_t)7;
        cap = off + 8 * n;
        pr = cap + 4 * n;
        grp = pr + sizeof(PrObj) * n;
        meta = grp + 4 * n;
        end = meta + 8 * n;
    }
    size_t alloc_bytes() const { return end + 64; }  // (never empty)
    // what the host uploads after the readback: [big, end)
    size_t upload_bytes() const { return end - big; }
    ClsView view(void *base) const {
        char *b = static_cast<char *>(base);
        const prk::MaxactView m = MaxactLayout{n}.view(b);
        return ClsView{m.most,
                       m.rows,
                       m.ents,
                       reinterpret_cast<uint32_t *>(b + big),
                       reinterpret_cast<unsigned long long *>(b + off),
                       reinterpret_cast<uint32_t *>(b + cap),
                       reinterpret_cast<PrObj *>(b + pr),
                       reinterpret_cast<uint32_t *>(b + grp),
                       reinterpret_cast<uint32_t *>(b + meta)};
    }
};

}  // namespace

extern "C" {

// ---- the span pass (flush_spans) and its phases ----------------------------
namespace {
struct HandleRun {  // a prk_draw_span_records draw: its launch after the thread walks
    uint32_t draw, g0, obj0, first, n;
    const void *sp;
};
// Walk groups: per mode, the large objects by the workgroup their list needs
// (slot_threads(lcap) >= most + 2, lcap <= the device's), the rest (more than
// lcap, or rows past k_obj_maxact's histogram) the huge-object walk or one
// wave each with the list in a pool slice.
struct WalkGroup {
    int32_t mode;
    uint32_t lcap, start, count;
    bool big;           // the huge-object walk (k_obj_walk_big / k_obj_walk_lds)
    uint32_t max_rows;  // (big: its objects' most rows)
    bool lds;           // (big: the list in LDS, k_obj_walk_lds)
};
// The chunked walk's groups: its objects by (mode, LDS capacity class).
struct PrGroup {
    int32_t mode;
    uint32_t cap, start, count, max_chunks;
};
// What classify() decides about a pass's large objects (with the h_cls tables).
struct ObjWalks {
    std::vector<WalkGroup> groups;
    std::vector<PrGroup> prgroups;
    uint64_t pool = 0;  // the pool slices' ints
    uint32_t npr = 0, pr_rows = 0, pr_chunks = 0, pr_max_edges = 0;  // the chunked walk's objects, rows, chunks
    uint64_t pr_ents = 0;
};
// The large objects of a pass by mode (the object, its edges), and as the
// readback lists them: mode after mode (SpanScratch h_big_gl's order).
struct BigObjs {
    std::vector<uint32_t> obj[prk::MODE_COUNT], edges[prk::MODE_COUNT];
    std::vector<uint32_t> all_edges;
};
// A host table of the pass in the pinned staging, and where the one upload puts it.
struct StagePart {
    const void *src = nullptr;
    size_t bytes = 0, off = 0;
};

// The walk groups of a pass, from what k_obj_maxact read back (h.most, rows,
// ents): the objects of every group into h.big / off / cap / meta, one group
// after the other.  Objects whose lists outgrow the slot walk's LDS classes
// take the huge-object walk (a workgroup of 1024: k_obj_walk_lds with the
// whole list in LDS when it fits prk_big_lds_cap() entries, else
// k_obj_walk_big with it in device memory) when their sizes are known and
// fit, else one wave each (k_obj_walk_wave).
static void classify_walks(const SpanSwitches &sw, uint32_t lcap, const BigObjs &B, const ClsView &h, ObjWalks &out,
                           uint32_t routes[9]) {
    uint32_t k = 0, b = 0;
    for (int mo = 0; mo < prk::MODE_COUNT; ++mo) {
        const std::vector<uint32_t> &objs = B.obj[mo];
        const uint32_t b0 = b;
        for (int ci = 0; ci <= 7; ++ci) {  // ci 5 / 6: the huge-object walk in LDS / device memory, 7: one wave each
            const uint32_t capc = ci < 5 ? kAdvWgCaps[ci] : 0u;
            if (ci < 5 && capc > lcap) continue;
            const uint32_t start = k;
            uint32_t gmax = 0;  // (the huge walk: its objects' most rows)
            for (uint32_t i = 0; i < objs.size(); ++i) {
                const uint32_t bi = b0 + i;
                const int32_t most = h.most[bi];
                // (big_min is a test switch of these groups alone: it sends
                // objects that fit a slot class to the walks past them; the
                // chunked walk's groups keep the plain rule)
                if ((most <= sw.big_min ? slot_class(most, lcap) : 0u) != capc) continue;
                const int32_t rows = h.rows[bi], ents = h.ents[bi];
                const bool huge = ci == 5 || ci == 6;
                if (ci >= 5) {
                    const bool hb = sw.big && most > 0 && (uint32_t)most <= prk_big_max_entries() && rows > 0 &&
                                    rows < INT32_MAX && ents >= 0 && ents < INT32_MAX && objs.size() <= 65535;
                    const bool hl = hb && sw.ldswalk && (uint32_t)most <= prk_big_lds_cap() && rows < 16000;
                    if ((hb ? (hl ? 5 : 6) : 7) != ci) continue;
                }
                const uint32_t cap = huge ? (uint32_t)most : B.edges[mo][i];
                if (huge) out.pool = (out.pool + 3) & ~3ull;  // (16-B aligned slices)
                h.big[k] = objs[i];
                h.off[k] = capc ? 0ull : out.pool;
                h.cap[k] = capc ? 0u : cap;
                h.meta[2 * k] = huge ? (uint32_t)rows : 0u;
                h.meta[2 * k + 1] = huge ? (uint32_t)ents : 0u;
                if (!capc)
                    out.pool += huge ? prk_big_slice_ints(cap, (uint32_t)rows, (uint32_t)ents)
                                     : (uint64_t)kWaveListArrays * (cap + 2);
                if (huge) gmax = std::max(gmax, (uint32_t)rows);
                ++routes[ci];
                ++k;
            }
            if (k > start) out.groups.push_back(WalkGroup{mo, capc, start, k - start, ci == 5 || ci == 6, gmax, ci == 5});
        }
        b += (uint32_t)objs.size();
    }
}

// The chunked walk (prk_spans.hip k_pr_*): the large objects walked with
// their lists in LDS whose rows fit its histogram, by (mode, slot class) as
// the walk groups; its table into h.pr, its objects by group into h.grp.
static void classify_chunked(const SpanSwitches &sw, uint32_t lcap, const BigObjs &B, const std::vector<uint32_t> &big_gl,
                      const ClsView &h, ObjWalks &out) {
    const uint32_t K = prk_pr_chunk_rows();
    uint32_t b = 0;
    for (int mo = 0; sw.rows && mo < prk::MODE_COUNT; ++mo) {
        const uint32_t b0 = b;
        for (const uint32_t capc : kAdvWgCaps) {
            if (capc > lcap) continue;
            PrGroup g{mo, capc, out.npr, 0, 0};
            for (uint32_t i = 0; i < B.obj[mo].size(); ++i) {
                const uint32_t bi = b0 + i;
                const int32_t most = h.most[bi], rows = h.rows[bi];
                if (most <= 0 || most > prk_pr_max_row_entries() || rows <= 0 || rows > prk_pr_max_rows()) continue;
                if (slot_class(most, lcap) != capc) continue;
                const uint32_t nch = ((uint32_t)rows + K - 1) / K;
                const uint64_t ents = (uint64_t)most * nch;
                if (out.pr_ents + ents > kPrMaxEntries || out.npr >= 65535 ||
                    (uint64_t)out.pr_rows + rows + 1 > 0x7FFFFFFFull)
                    continue;
                PrObj &q = h.pr[out.npr];
                q.o = big_gl[bi];
                q.row_off = out.pr_rows;
                q.rows = (uint32_t)rows;
                q.chunk_off = out.pr_chunks;
                q.most = (uint32_t)most;
                q.ent_off = (uint32_t)out.pr_ents;
                q.pad0 = q.pad1 = 0;
                h.grp[out.npr] = out.npr;
                out.pr_rows += (uint32_t)rows + 1;
                out.pr_chunks += nch;
                out.pr_ents += ents;
                out.pr_max_edges = std::max(out.pr_max_edges, B.all_edges[bi]);
                g.max_chunks = std::max(g.max_chunks, nch);
                ++g.count;
                ++out.npr;
            }
            if (g.count) out.prgroups.push_back(g);
        }
        b += (uint32_t)B.obj[mo].size();
    }
}

// One span pass: what its phases share.  flush_spans runs them in order.
struct SpanPass {
    prk_context *c;
    prk_context::SpanScratch &S;
    hipStream_t s;
    const std::vector<prk::DrawRec> &draws;
    const SpanSwitches sw;
    prk::FrameParams fp;
    uint32_t ntiles = 0;
    uint32_t lcap = 0;  // LDS list capacity of the wave walk (edges)
    // plan(): objects, kind-0 objects, triangles; the prk_draw_edges edges.
    // The pass's batches (prk_draw_edge_lists) take consecutive records and
    // lists of the frame's: [le0, le0 + nhe) and [ll0, ll0 + nhl).  With the
    // handle draws' (prk_draw_records) the pass has nle batch edges and nll
    // batch lists, in submission order.
    uint32_t nobj = 0, nk0 = 0, nt = 0, nbig = 0, le0 = 0, ll0 = 0, nsegblk = 0;
    uint64_t nk1 = 0, nle = 0, nll = 0, nhe = 0, nhl = 0;
    uint64_t maxn = 1, small_tris = 0, small_ledges = 0;
    uint32_t pbits = 0, ybits = 0, obits = 0;  // MergeSort key: (object, min(YMin, H), recursion path)
    bool handles = false;                      // a pass with handle draws (prk_draw_records)
    bool thread_links = false;  // a thread-walked triangle object small enough for LDS list links
    BigObjs big;
    std::vector<HandleRun> hruns;
    std::vector<uint8_t> seg_staged;  // per h_segs segment: its records are staged ones
    // upload(): the staged tables, in the staging's order
    StagePart st_draws, st_texs, st_runs, st_big, st_k1src, st_edges, st_spans, st_lcnt, st_lflag, st_ledges, st_lseg,
        st_lsrc;
    // edges(): the pass's span kinds (bit per Mode), the sort and the small objects' walk
    uint32_t modes = 0;
    bool scalar = false, local_sort = false, segmented = false;
    uint64_t max_segs = 0;
    ObjDesc *d_objs = nullptr;
    uint32_t *escan = nullptr;
    const uint32_t *total0p = nullptr;
    unsigned long long *oslot = nullptr;
    // sizes(): the span slots; the classification block
    uint32_t nslot = 0;
    ClsLayout cls;
    ObjWalks walks;
    const uint32_t *d_prstat = nullptr;  // the chunked walk ran: its objects' status

    SpanPass(prk_context *ctx, hipStream_t stream, const std::vector<prk::DrawRec> &d)
        : c(ctx), S(ctx->spans), s(stream), draws(d) {}
    void *dev(const StagePart &p) const { return S.d_stage.as<char>() + p.off; }
    ScSpanRec *srecs() const { return scalar ? S.d_srecs.as<ScSpanRec>() : nullptr; }  // DrawModel span records
    int2 *wy() const { return segmented ? S.d_wy.as<int2>() : nullptr; }
    int plan();
    int upload();
    int edges();
    int sizes();
    void classify();
    int chunked();
    int walk();
    int bin_shade(uint32_t T);
};

// The loop over the draws, host only.  Objects in submission order (ObjDesc
// kinds: prk_spans.hip): kind 0 objects' triangles numbered 0..ntri-1 in order
// (FillEdgeTable runs per triangle), caller edge lists' edges after the
// triangles' edges.  Objects of kObjWaveTris triangles or more are large.
// (the objects themselves are expanded on the device from runs: a draw of
// kind 0 is a run of ceil(tris / obj_tris) objects, kind 2 one of its spans;
// only the large objects are listed here)
int SpanPass::plan() {
    S.h_runs.clear();
    S.h_big_gl.clear();
    S.h_k1src.clear();
    S.h_segs.clear();
    S.h_lsrc.clear();
    uint64_t ntri = 0, nobj64 = 0, nk064 = 0;
    for (const prk::DrawRec &d : draws) handles = handles || d.src_kind == 4;
    // only a pass with handle draws lists the segments of its batch edges
    // (h_segs; a staged segment's src: its record among the staged ones, until
    // the staging has its address)
    auto add_seg = [&](uint64_t src, bool staged, uint32_t n) {
        if (!handles || !n) return;
        if (!S.h_segs.empty() && seg_staged.back() == (staged ? 1 : 0) &&
            reinterpret_cast<uintptr_t>(S.h_segs.back().src) + sizeof(prk_edge) * (uint64_t)S.h_segs.back().n == src) {
            S.h_segs.back().n += n;  // (the records go on where the previous segment's end)
            return;
        }
        S.h_segs.push_back(PrepSeg{reinterpret_cast<const uint32_t *>(src), (uint32_t)nle, n, 0u, 0u});
        seg_staged.push_back(staged ? 1 : 0);
    };
    for (uint32_t di = 0; di < draws.size(); ++di) {
        const prk::DrawRec &d = draws[di];
        if (d.src_kind == 1) {
            S.h_runs.push_back(ObjRun{1u, di, (uint32_t)nobj64, 1u, 0u, 0u, d.first_global, 0u, 0u, d.src_off, d.src_n,
                                      (uint32_t)nk1});
            for (uint32_t e = 0; e < d.src_n; ++e) S.h_k1src.push_back(d.src_off + e);
            nk1 += d.src_n;
            nobj64 += 1;
        } else if (d.src_kind == 2) {
            if (!d.src_n) continue;
            S.h_runs.push_back(ObjRun{2u, di, (uint32_t)nobj64, d.src_n, 0u, 0u, d.first_global, 0u, 0u, d.src_off, 0u, 0u});
            nobj64 += d.src_n;
        } else if (d.src_kind == 5) {
            // the spans stay where they are: a run of one-slot objects that
            // k_span_handle_walk fills from the handle's buffer
            if (!d.src_n) continue;
            S.h_runs.push_back(ObjRun{4u, di, (uint32_t)nobj64, d.src_n, 0u, 0u, d.first_global, 0u, 0u, d.src_off, 0u, 0u});
            hruns.push_back(HandleRun{di, d.first_global, (uint32_t)nobj64, d.src_off, d.src_n, c->sbatches[d.geom].sp});
            nobj64 += d.src_n;
        } else if (d.src_kind == 3 || d.src_kind == 4) {
            // one run for the batch; its sorted lists are routed like triangle
            // objects of as many edges (k1off: the first batch edge's slot, below).
            // The run's list tables: `per` on in the staged ones (tri0 0), or
            // in those of handle source tri0 - 1 (k_list_tables).
            const uint32_t *lcnt, *lflag;
            uint32_t src = 0, at;
            if (d.src_kind == 3) {
                if (!nhl) {
                    le0 = d.src_off;
                    ll0 = d.geom_tri0;
                }
                lcnt = c->pend_lcnt.data() + d.geom_tri0;
                lflag = c->pend_lflag.data() + d.geom_tri0;
                at = (uint32_t)nhl;
                add_seg(sizeof(prk_edge) * nhe, true, d.src_n);
                nhl += d.tri_count;
                nhe += d.src_n;
            } else {
                const Records &R = c->recs[d.geom];
                lcnt = R.cnt.data() + d.geom_tri0;
                lflag = R.flag.data() + d.geom_tri0;
                at = d.geom_tri0;
                for (src = 0; src < S.h_lsrc.size() && S.h_lsrc[src].cnt != R.d_cnt(); ++src) {}
                if (src == S.h_lsrc.size()) S.h_lsrc.push_back(ListSrc{R.d_cnt(), R.d_flag()});
                ++src;
                add_seg(reinterpret_cast<uintptr_t>(R.rec) + sizeof(prk_edge) * (uint64_t)d.src_off, false, d.src_n);
            }
            S.h_runs.push_back(ObjRun{3u, di, (uint32_t)nobj64, d.tri_count, handles ? at : 0u, 0u, d.first_global,
                                      src, (uint32_t)nll, 0u, 0u, 0u});
            for (uint32_t j = 0; j < d.tri_count; ++j) {
                const uint32_t n = lcnt[j];
                if (!lflag[j]) continue;
                if (n >= kObjWaveEdges) {
                    big.obj[d.mode].push_back((uint32_t)(nobj64 + j));
                    big.edges[d.mode].push_back(n);
                } else {
                    small_ledges += n;
                    thread_links = thread_links || (n && n <= prk_obj_link_cap());
                }
            }
            nobj64 += d.tri_count;
            nll += d.tri_count;
            nle += d.src_n;
        } else {
            const uint32_t per = std::max<uint32_t>(1u, d.obj_tris);
            const uint32_t cnt = (uint32_t)(((uint64_t)d.tri_count + per - 1) / per);
            if (!cnt) continue;
            S.h_runs.push_back(ObjRun{0u, di, (uint32_t)nobj64, cnt, per, d.tri_count, d.first_global, (uint32_t)ntri,
                                      (uint32_t)nk064, 0u, 0u, 0u});
            maxn = std::max<uint64_t>(maxn, 3ull * std::min(per, d.tri_count));  // the most its FillEdgeTable writes
            if (per >= kObjWaveTris) {
                for (uint32_t j = 0; j < cnt; ++j) {
                    const uint32_t n = std::min(per, d.tri_count - j * per);
                    if (n >= kObjWaveTris) {
                        big.obj[d.mode].push_back((uint32_t)(nobj64 + j));
                        big.edges[d.mode].push_back(3u * n);
                    } else {
                        small_tris += n;
                        thread_links = thread_links || 3ull * n <= prk_obj_link_cap();
                    }
                }
            } else {
                const uint32_t rem = d.tri_count % per;
                small_tris += d.tri_count;
                thread_links = thread_links || (d.tri_count >= per && 3ull * per <= prk_obj_link_cap()) ||
                               (rem && 3ull * rem <= prk_obj_link_cap());
            }
            nobj64 += cnt;
            nk064 += cnt;
            ntri += d.tri_count;
        }
        if (nobj64 >= 0x7FFFFFFFull) return PRK_ERR_LIMIT;
    }
    for (int mo = 0; mo < prk::MODE_COUNT; ++mo)  // the large objects, by mode (their walk groups: after the readback)
        for (size_t i = 0; i < big.obj[mo].size(); ++i) {
            S.h_big_gl.push_back(big.obj[mo][i]);
            big.all_edges.push_back(big.edges[mo][i]);
        }
    // edge slots (3 per triangle + the caller edges) are indexed by 31 bits
    if (3 * ntri + nk1 + nle >= 0x7FFFFFFFull) return PRK_ERR_LIMIT;
    for (ObjRun &r : S.h_runs)  // the batch edges' slots follow the prk_draw_edges lists'
        if (r.kind == 3) r.k1off = (uint32_t)nk1;
    S.h_lcnt.assign(c->pend_lcnt.begin() + ll0, c->pend_lcnt.begin() + ll0 + nhl);
    S.h_lcnt.push_back(0u);  // (the scan's total)
    for (PrepSeg &sg : S.h_segs) {
        sg.blk0 = nsegblk;
        nsegblk += (sg.n + kPrepEdges - 1) / kPrepEdges;
    }
    nobj = (uint32_t)nobj64;
    nk0 = (uint32_t)nk064;
    nt = (uint32_t)ntri;
    nbig = (uint32_t)S.h_big_gl.size();
    // MergeSort key: (object, min(YMin, H), recursion path) in one radix sort
    auto bitlen = [](uint64_t v) { uint32_t b = 0; while (v) { ++b; v >>= 1; } return b; };
    pbits = bitlen(maxn) + 1;
    ybits = std::max(1u, bitlen((uint64_t)c->H));
    obits = std::max(1u, bitlen(nk0 > 0 ? nk0 - 1 : 0));
    if (obits + ybits + pbits > 64) return PRK_ERR_LIMIT;
    tex_table(c, S.h_texs);
    S.h_draws = draws;
    return PRK_OK;
}

// The pass's host tables go up in one copy from pinned staging (a pageable
// hipMemcpyAsync per table held the host for each).
// (the scratch is reused frame to frame: stream order on s covers it)
int SpanPass::upload() {
    st_draws = {S.h_draws.data(), S.h_draws.size() * sizeof(prk::DrawRec)};
    st_texs = {S.h_texs.data(), S.h_texs.size() * sizeof(prk::TexRec)};
    st_runs = {S.h_runs.data(), S.h_runs.size() * sizeof(ObjRun)};
    st_big = {S.h_big_gl.data(), S.h_big_gl.size() * 4};
    st_k1src = {S.h_k1src.data(), S.h_k1src.size() * 4};
    st_edges = {c->pend_edges.data(), c->pend_edges.size() * sizeof(prk_edge)};
    st_spans = {c->pend_spans.data(), c->pend_spans.size() * sizeof(prk_span)};
    st_lcnt = {S.h_lcnt.data(), nhl ? S.h_lcnt.size() * 4 : 0};
    st_lflag = {c->pend_lflag.data() + ll0, (size_t)nhl * 4};
    st_ledges = {c->pend_ledges.data() + le0, (size_t)nhe * sizeof(prk_edge)};
    st_lseg = {S.h_segs.data(), S.h_segs.size() * sizeof(PrepSeg)};
    st_lsrc = {S.h_lsrc.data(), S.h_lsrc.size() * sizeof(ListSrc)};
    StagePart *parts[] = {&st_draws, &st_texs,  &st_runs,   &st_big,  &st_k1src, &st_edges,
                          &st_spans, &st_lcnt, &st_lflag, &st_ledges, &st_lseg, &st_lsrc};
    size_t stage_bytes = 0;
    for (StagePart *pt : parts) {
        pt->off = stage_bytes;
        stage_bytes = (stage_bytes + pt->bytes + 255) & ~(size_t)255;
    }
    stage_bytes = std::max<size_t>(stage_bytes, 256);
    S.last_stage_bytes = stage_bytes;
    if (!S.stage_ev) PRK_TRY(hipEventCreateWithFlags(&S.stage_ev, hipEventDisableTiming));
    if (S.stage_busy) {  // the previous pass's upload still reads the staging
        PRK_TRY(hipEventSynchronize(S.stage_ev));
        S.stage_busy = false;
    }
    if (stage_bytes > S.stage_cap) {
        if (S.h_stage) (void)hipHostFree(S.h_stage);
        S.h_stage = nullptr;
        S.stage_cap = 0;
        const size_t want = stage_bytes + stage_bytes / 4;
        PRK_TRY(hipHostMalloc((void **)&S.h_stage, want, hipHostMallocDefault));
        S.stage_cap = want;
    }
    PRK_TRY(S.d_stage.ensure(stage_bytes));
    for (size_t i = 0; i < S.h_segs.size(); ++i)  // the staged segments' records, where the staging puts them
        if (seg_staged[i])  // (src held the record's byte offset till now)
            S.h_segs[i].src = reinterpret_cast<const uint32_t *>(static_cast<const char *>(dev(st_ledges)) +
                                                                 reinterpret_cast<uintptr_t>(S.h_segs[i].src));
    for (const StagePart *pt : parts)
        if (pt->bytes && pt->src) std::memcpy(S.h_stage + pt->off, pt->src, pt->bytes);
    PRK_TRY(hipMemcpyAsync(S.d_stage.p, S.h_stage, stage_bytes, hipMemcpyHostToDevice, s));
    PRK_TRY(hipEventRecord(S.stage_ev, s));
    S.stage_busy = true;
    fp.draws = (const prk::DrawRec *)dev(st_draws);
    fp.texs = (const prk::TexRec *)dev(st_texs);
    fp.draw0 = draws[0];
    fp.tex0 = prk::TexRec{};
    if (fp.draw0.tex >= 0 && (size_t)fp.draw0.tex < S.h_texs.size()) fp.tex0 = S.h_texs[fp.draw0.tex];
    return PRK_OK;
}

// The object tables, FillEdgeTable per triangle (counts, scans, edges +
// MergeSort keys), the sort, the walk's working copy, each object's bound
// and its scan into the objects' first span slots.
int SpanPass::edges() {
    // the objects (ObjDesc), the kind-0 objects' indices and first triangles
    PRK_TRY(S.d_objtab.ensure_n<ObjDesc>(std::max<uint32_t>(nobj, 1)));
    PRK_TRY(S.d_k0tab.ensure((size_t)std::max<uint32_t>(nk0, 1) * 8));
    d_objs = S.d_objtab.as<ObjDesc>();
    uint32_t *k0tab = (uint32_t *)S.d_k0tab.p;
    const uint32_t *d_k0obj = k0tab, *d_k0tri0 = k0tab + nk0;
    // the batch lists' first edges: the scan of their counts
    const uint32_t nlist = (uint32_t)nll, nledge = (uint32_t)nle;
    uint32_t *lscan = nullptr, *lobj = nullptr;
    const uint32_t *d_lcnt = (const uint32_t *)dev(st_lcnt), *d_lflag = (const uint32_t *)dev(st_lflag);
    if (nlist) {
        PRK_TRY(S.d_lscan.ensure(((size_t)nlist + 1) * 4));
        PRK_TRY(S.d_lobj.ensure((size_t)nlist * 4));
        PRK_TRY(S.d_lrows.ensure((size_t)nlist * 8));
        lscan = (uint32_t *)S.d_lscan.p;
        lobj = (uint32_t *)S.d_lobj.p;
        if (handles) {  // the lists' tables from their sources, on the device
            PRK_TRY(S.d_ltab.ensure((2 * (size_t)nlist + 1) * 4));
            uint32_t *lt = (uint32_t *)S.d_ltab.p;
            PRK_TRY(prk_list_tables(static_cast<const ObjRun *>(dev(st_runs)), (uint32_t)S.h_runs.size(), nobj, d_lcnt,
                                    d_lflag, static_cast<const ListSrc *>(dev(st_lsrc)), nlist, lt, lt + nlist + 1, s));
            d_lcnt = lt;
            d_lflag = lt + nlist + 1;
        }
        PRK_TRY(scan_u32(S.d_temp, d_lcnt, lscan, nlist + 1, s));
    }
    PRK_TRY(prk_obj_tables(static_cast<const ObjRun *>(dev(st_runs)), (uint32_t)S.h_runs.size(), nobj, kObjWaveTris,
                           d_objs, k0tab, k0tab + nk0, d_lcnt, d_lflag, lscan, kObjWaveEdges, lobj, s));
    const uint32_t *d_k1src = (const uint32_t *)dev(st_k1src);
    for (const auto &d : draws) modes |= 1u << d.mode;
    scalar = (modes & ~(1u << prk::MODE_AVX)) != 0;
    // FillEdgeTable per triangle: counts, scans, edges + MergeSort keys.
    const size_t es = std::max<size_t>(3 * (size_t)nt, 1);
    PRK_TRY(S.d_ecnt.ensure(((size_t)nt + 1) * 4));
    PRK_TRY(S.d_escan.ensure(((size_t)nt + 1) * 4));
    PRK_TRY(S.d_rcnt.ensure(((size_t)nt + 1) * 8));
    PRK_TRY(S.d_rscan.ensure(((size_t)nt + 1) * 8));
    PRK_TRY(S.d_edges.ensure_n<ObjEdge>(es));
    PRK_TRY(S.d_ekeys.ensure(es * 8));
    PRK_TRY(S.d_ekeys2.ensure(es * 8));
    PRK_TRY(S.d_evals.ensure(es * 4));
    PRK_TRY(S.d_ord.ensure(es * 4));
    PRK_TRY(S.d_err.ensure(16));
    PRK_TRY(hipMemsetAsync(S.d_err.p, 0, 16, s));  // (error bits, then the chunked walk's tally)
    escan = (uint32_t *)S.d_escan.p;
    uint32_t *ord = (uint32_t *)S.d_ord.p;
    ObjEdge *d_edges = S.d_edges.as<ObjEdge>();
    unsigned long long *ekeys = S.d_ekeys.as<unsigned long long>();
    unsigned long long *rscan = (unsigned long long *)S.d_rscan.p;
    total0p = escan + nt;
    if (nt) {
        PRK_TRY(prk_objtri_count(&fp, d_objs, d_k0obj, d_k0tri0, nk0,
                                 nt, (uint32_t *)S.d_ecnt.p, (unsigned long long *)S.d_rcnt.p, s));
    } else {
        PRK_TRY(hipMemsetAsync(S.d_ecnt.p, 0, 4, s));
        PRK_TRY(hipMemsetAsync(S.d_rcnt.p, 0, 8, s));
    }
    PRK_TRY(scan_u32(S.d_temp, (const uint32_t *)S.d_ecnt.p, escan, nt + 1, s));
    PRK_TRY(scan_u64(S.d_temp, (const unsigned long long *)S.d_rcnt.p, rscan, nt + 1, s));
    // MergeSort of every object: per object when none has more than 64
    // edges (k_obj_sort_local, with the gather), else one radix sort of the
    // padded keys (prk_spans.hip)
    local_sort = nt && maxn <= 64 && sw.local_sort;
    PRK_TRY(prk_objtri_emit(&fp, d_objs, d_k0obj, d_k0tri0, nk0, nt, escan, pbits, ybits, c->H, d_edges, ekeys,
                            (uint32_t *)S.d_evals.p, local_sort ? 0 : 1, s));
    if (nt && !local_sort)
        PRK_TRY(obj_sort(S.d_temp, ekeys, (uint32_t *)S.d_evals.p, S.d_ekeys2.p, ord, 3 * nt,
                         obits + ybits + pbits, s));
    PRK_TRY(S.d_bound.ensure(((size_t)nobj + 1) * 8));
    PRK_TRY(S.d_oslot.ensure(((size_t)nobj + 1) * 8));
    oslot = (unsigned long long *)S.d_oslot.p;
    // The walk's working copy (the triangle edges, the prk_draw_edges lists,
    // the batch lists).
    const uint32_t nwork = 3 * nt + (uint32_t)nk1 + nledge;
    PRK_TRY(S.d_work.ensure_n<ObjEdge>(std::max<size_t>(nwork, 1)));
    ObjEdge *work = S.d_work.as<ObjEdge>();
    // The small triangle objects' segments (prk_spans.hip k_obj_seg, walk()):
    // a thread per stretch of rows with a non-empty list.
    max_segs = 3 * small_tris + small_ledges;  // (a segment has an edge at least)
    segmented = max_segs && max_segs < 0x7FFFFFFFull && sw.segments;
    if (segmented) PRK_TRY(S.d_wy.ensure((size_t)std::max<uint32_t>(nwork, 1) * 8));
    if (local_sort)
        PRK_TRY(prk_obj_sort_local(d_objs, d_k0obj, nk0, escan, ekeys, d_edges, work, wy(),
                                   (uint32_t *)S.d_err.p, s));
    if (!local_sort || nk1)
        PRK_TRY(prk_obj_gather(d_edges, local_sort ? nullptr : ord, total0p,
                               static_cast<const EdgeIn *>(dev(st_edges)), d_k1src,
                               (uint32_t)nk1, work, 3 * nt + (uint32_t)nk1, wy(), s));
    // the batch lists' records into it, with their lists' row sums; then the
    // span slots: each object's bound, exclusive-scanned into its first slot
    if (handles)
        PRK_TRY(prk_list_prep_segs(&fp, static_cast<const PrepSeg *>(dev(st_lseg)), (uint32_t)S.h_segs.size(), nsegblk,
                                   lscan, nlist, lobj,
                                   d_objs, total0p, (uint32_t)nk1, work, wy(), (unsigned long long *)S.d_lrows.p, s));
    else
        PRK_TRY(prk_list_prep(&fp, dev(st_ledges), nledge, lscan, nlist, lobj, d_objs, total0p, (uint32_t)nk1,
                              work, wy(), (unsigned long long *)S.d_lrows.p, s));
    PRK_TRY(prk_obj_bound(&fp, d_objs, nobj, rscan, static_cast<const EdgeIn *>(dev(st_edges)),
                          (const unsigned long long *)S.d_lrows.p, (unsigned long long *)S.d_bound.p, s));
    PRK_TRY(scan_u64(S.d_temp, (const unsigned long long *)S.d_bound.p, oslot, nobj + 1, s));
    return PRK_OK;
}

// Each large object's most active edges, rows and entries (they size its
// walk), read back with the slot total: the pass's first wait.  Then the
// span slots' buffers.
int SpanPass::sizes() {
    cls = ClsLayout(nbig);
    if (cls.alloc_bytes() > S.cls_cap) {
        if (S.h_cls) (void)hipHostFree(S.h_cls);
        S.h_cls = nullptr;
        S.cls_cap = 0;
        const size_t want = cls.alloc_bytes() + cls.alloc_bytes() / 4;
        PRK_TRY(hipHostMalloc((void **)&S.h_cls, want, hipHostMallocDefault));
        S.cls_cap = want;
    }
    const size_t most_bytes = MaxactLayout{nbig}.bytes();
    if (nbig) {
        const uint32_t *d_big = (const uint32_t *)dev(st_big);
        PRK_TRY(S.d_most.ensure(most_bytes));
        PRK_TRY(prk_obj_maxact(&fp, d_objs, d_big, nbig, escan, total0p, S.d_work.as<ObjEdge>(), S.d_most.as<int32_t>(),
                               sw.huge_edges, s));
        for (uint32_t &r : S.walk_routes) r = 0;  // (prk_debug_walk_routes: this pass's)
        for (uint32_t b = 0; b < nbig; ++b)  // (objects of sw.huge_edges edges or more: many workgroups each)
            if (big.all_edges[b] >= sw.huge_edges) {
                ++S.walk_routes[8];
                PRK_TRY(S.d_mhuge.ensure(prk_maxact_huge_scratch()));
                PRK_TRY(prk_obj_maxact_huge(&fp, d_objs, d_big, b, nbig, big.all_edges[b], escan, total0p,
                                            S.d_work.as<ObjEdge>(), S.d_most.as<int32_t>(), S.d_mhuge.p, s));
            }
        PRK_TRY(hipMemcpyAsync(S.h_cls, S.d_most.p, most_bytes, hipMemcpyDeviceToHost, s));
    }
    PRK_TRY(hipMemcpyAsync(S.h_rb, oslot + nobj, 8, hipMemcpyDeviceToHost, s));
    PRK_TRY(hipStreamSynchronize(s));
    uint64_t nslot64;
    std::memcpy(&nslot64, S.h_rb, 8);
    if (nslot64 >= prk::kMaxPairs) return PRK_ERR_LIMIT;  // 31-bit span tags
    nslot = (uint32_t)nslot64;
    const size_t ns = std::max<uint32_t>(nslot, 1);
    PRK_TRY(S.d_recs.ensure_n<SpanRec>(ns));
    PRK_TRY(S.d_pos.ensure_n<SpanPos>(ns));
    PRK_TRY(S.d_span_tri.ensure(ns * 4));
    if (scalar) PRK_TRY(S.d_srecs.ensure_n<ScSpanRec>(ns));
    if (nbig) PRK_TRY(S.d_raw.ensure_n<PairRaw>(ns));  // the slot walks' pairs
    // slots no span takes stay row -1: binned nowhere.  Without large objects
    // every slot belongs to the thread or segment walks (walk_object,
    // k_obj_seg), which mark their unused ones themselves (C3b as 16-triangle
    // objects: ~21 M slots, a 0.34-GB memset); the large objects' walks rely
    // on this one.
    if (nbig || sw.pos_memset) PRK_TRY(hipMemsetAsync(S.d_pos.p, 0xFF, ns * sizeof(SpanPos), s));
    return PRK_OK;
}

// The large objects' walks from the readback, on the host alone.
void SpanPass::classify() {
    const ClsView h = cls.view(S.h_cls);
    if (nbig) {
        S.walk_sizes[0] = h.most[0];
        S.walk_sizes[1] = h.rows[0];
        S.walk_sizes[2] = h.ents[0];
    }
    classify_walks(sw, lcap, big, h, walks, S.walk_routes);
    classify_chunked(sw, lcap, big, S.h_big_gl, h, walks);
}

// The chunked walk of the objects classify() gave it.  It is an
// optimisation: when its scratch (up to kPrMaxEntries * ~356 B) cannot be
// had, every object takes the workgroup walk instead (d_prstat stays null) --
// never PRK_ERR_NOMEM.
int SpanPass::chunked() {
    ObjWalks &w = walks;
    if (!w.npr) return PRK_OK;
    hipError_t ae = S.d_prstat.ensure((size_t)nobj * 4);
    if (ae == hipSuccess) ae = S.d_prrow.ensure_n<PrRow>(w.npr);
    if (ae == hipSuccess) ae = S.d_prcnt.ensure((size_t)w.pr_rows * 4);
    if (ae == hipSuccess) ae = S.d_preoff.ensure((size_t)w.pr_rows * 4);
    if (ae == hipSuccess) ae = S.d_prfge.ensure((size_t)w.pr_rows * 4);
    if (ae == hipSuccess) ae = S.d_prccur.ensure((size_t)w.pr_chunks * 4);
    if (ae == hipSuccess) ae = S.d_preendm.ensure((size_t)w.pr_chunks * 4);
    if (ae == hipSuccess) ae = S.d_prmatch.ensure((size_t)w.pr_chunks * 4);
    if (ae == hipSuccess) ae = S.d_prsm.ensure((size_t)w.pr_chunks * 4);
    if (ae == hipSuccess) ae = S.d_prsidx.ensure(w.pr_ents * 4);
    if (ae == hipSuccess) ae = S.d_prkey.ensure_n<float4>(w.pr_ents);
    if (ae == hipSuccess) ae = S.d_prest.ensure_n<ObjEdge>(w.pr_ents);
    if (ae == hipSuccess) ae = S.d_prsst.ensure_n<ObjEdge>(w.pr_ents);
    if (ae == hipSuccess) ae = S.d_preend.ensure_n<ObjEdge>(w.pr_ents);
    if (ae == hipErrorOutOfMemory) {
        (void)hipGetLastError();
        DevBuf *bufs[] = {&S.d_prsidx, &S.d_prkey, &S.d_prest, &S.d_prsst, &S.d_preend};
        for (DevBuf *b : bufs) b->release();
        w.npr = 0;
        return PRK_OK;
    }
    PRK_TRY(ae);
    PRK_TRY(hipMemsetAsync(S.d_prstat.p, 0, (size_t)nobj * 4, s));
    const ClsView d = cls.view(S.d_cls.p);
    prk::PrWalkArgs pa{};
    pa.objs = d_objs;
    pa.pro = d.pr;
    pa.npr = w.npr;
    pa.nchunks = w.pr_chunks;
    pa.max_edges = w.pr_max_edges;
    pa.escan = escan;
    pa.total0p = total0p;
    pa.work = S.d_work.as<ObjEdge>();
    pa.prrow = S.d_prrow.as<PrRow>();
    pa.cnt = (uint32_t *)S.d_prcnt.p;
    pa.eoff = (uint32_t *)S.d_preoff.p;
    pa.fge = (uint32_t *)S.d_prfge.p;
    pa.ccur = (uint32_t *)S.d_prccur.p;
    pa.key = S.d_prkey.as<float4>();
    pa.est = S.d_prest.as<ObjEdge>();
    pa.sst = S.d_prsst.as<ObjEdge>();
    pa.eend = S.d_preend.as<ObjEdge>();
    pa.eend_m = (uint32_t *)S.d_preendm.p;
    pa.match = (uint32_t *)S.d_prmatch.p;
    pa.sidx = (uint32_t *)S.d_prsidx.p;
    pa.s_m = (uint32_t *)S.d_prsm.p;
    pa.prstat = (uint32_t *)S.d_prstat.p;
    pa.soff = oslot;
    pa.raw = S.d_raw.as<PairRaw>();
    pa.pos = S.d_pos.as<SpanPos>();
    pa.span_tri = (uint32_t *)S.d_span_tri.p;
    pa.err = (uint32_t *)S.d_err.p;
    pa.warmup = sw.chunk_warmup;
    PRK_TRY(prk_pr_walk_begin(&fp, &pa, s));
    for (const PrGroup &g : w.prgroups)
        PRK_TRY(prk_pr_walk_group(&fp, &pa, g.mode, g.cap, d.grp + g.start, g.count, g.max_chunks, s));
    PRK_TRY(prk_pr_walk_end(&pa, s));
    d_prstat = (const uint32_t *)S.d_prstat.p;
    return PRK_OK;
}

// The classification's upload and every walk: the chunked walk, the small
// objects' segments and thread walk, the span handles, the walk groups; then
// the slot walks' pairs into span records.
int SpanPass::walk() {
    if (nbig) {
        PRK_TRY(S.d_cls.ensure(cls.end));
        PRK_TRY(hipMemcpyAsync(S.d_cls.as<char>() + cls.big, S.h_cls + cls.big, cls.upload_bytes(),
                               hipMemcpyHostToDevice, s));
        if (walks.pool) PRK_TRY(S.d_pool.ensure(walks.pool * 4));
    }
    {
        const int rc = chunked();
        if (rc != PRK_OK) return rc;
    }
    ObjEdge *work = S.d_work.as<ObjEdge>();
    SpanRecG *recs = S.d_recs.as<SpanRecG>();  // (the walks store a span record as its four quads)
    SpanPos *pos = S.d_pos.as<SpanPos>();
    PairRaw *raw = S.d_raw.as<PairRaw>();
    const ObjSeg *d_segs = nullptr;  // (the segments)
    const uint32_t *d_nseg = nullptr;
    if (segmented) {
        PRK_TRY(S.d_segcnt.ensure(((size_t)nobj + 1) * 4));
        PRK_TRY(S.d_segoff.ensure(((size_t)nobj + 1) * 4));
        PRK_TRY(S.d_segs.ensure_n<ObjSeg>(max_segs));
        uint32_t *segcnt = (uint32_t *)S.d_segcnt.p, *segoff = (uint32_t *)S.d_segoff.p;
        PRK_TRY(prk_obj_seg(&fp, d_objs, nobj, escan, total0p, wy(), oslot, segcnt, segoff, nullptr, nullptr, s));
        PRK_TRY(scan_u32(S.d_temp, segcnt, segoff, nobj + 1, s));
        PRK_TRY(prk_obj_seg(&fp, d_objs, nobj, escan, total0p, wy(), oslot, segcnt, segoff, S.d_segs.as<ObjSeg>(), pos,
                            s));
        d_segs = S.d_segs.as<ObjSeg>();
        d_nseg = segoff + nobj;
    }
    uint32_t *span_tri = (uint32_t *)S.d_span_tri.p, *err = (uint32_t *)S.d_err.p;
    PRK_TRY(prk_obj_walk(&fp, d_objs, nobj, escan, total0p, work, oslot, recs, srecs(), pos, span_tri,
                         static_cast<const prk::SpanIn *>(dev(st_spans)), err, thread_links ? 1 : 0, d_segs, d_nseg,
                         (uint32_t)max_segs, s));
    for (const HandleRun &h : hruns)  // the span handles' draws, from their own buffers
        PRK_TRY(prk_span_handle_walk(&fp, h.draw, h.g0, h.obj0, h.sp, h.first, h.n, oslot, recs, pos, span_tri, s));
    const ClsView d = cls.view(S.d_cls.p);
    for (const WalkGroup &g : walks.groups) {
        if (g.big)
            PRK_TRY(prk_big_walk(&fp, g.mode, g.lds ? 1 : 0, d_objs, d.big + g.start, d.off + g.start, d.cap + g.start,
                                 d.meta + 2 * (size_t)g.start, g.count, g.max_rows, (int32_t *)S.d_pool.p, escan,
                                 total0p, work, oslot, raw, pos, span_tri, err, d_prstat, s));
        else
            PRK_TRY(prk_obj_walk_group(&fp, g.mode, g.lcap, d_objs, d.big + g.start, d.off + g.start, d.cap + g.start,
                                       g.count, (int32_t *)S.d_pool.p, escan, total0p, work, oslot, recs, srecs(), raw,
                                       pos, span_tri, err, d_prstat, s));
    }
    if (nbig)  // the slot walks' pairs into span records
        PRK_TRY(prk_span_finish(&fp, raw, nslot, recs, srecs(), pos, s));
    return PRK_OK;
}

// span -> tile bin entries: the tiles' counts and their scan (the total comes
// back with the walks' status: the pass's second wait), then every span
// placed; visibility and shading.
int SpanPass::bin_shade(uint32_t T) {
    PRK_TRY(S.d_scnt.ensure(((size_t)ntiles + 1) * 4));
    PRK_TRY(S.d_offs.ensure(((size_t)ntiles + 1) * 4));
    uint32_t *tcnt = (uint32_t *)S.d_scnt.p, *toff = (uint32_t *)S.d_offs.p;
    PRK_TRY(prk_span_count(&fp, S.d_pos.as<SpanPos>(), nslot, tcnt, s));
    PRK_TRY(scan_u32(S.d_temp, tcnt, toff, ntiles + 1, s));
    PRK_TRY(hipMemcpyAsync(S.h_rb + 2, toff + ntiles, 4, hipMemcpyDeviceToHost, s));
    PRK_TRY(hipMemcpyAsync(S.h_rb + 3, S.d_err.p, 16, hipMemcpyDeviceToHost, s));
    PRK_TRY(hipStreamSynchronize(s));
    const uint32_t total = S.h_rb[2];
    if (S.h_rb[3]) return PRK_ERR_DEVICE;  // a walk outside its LDS list or span slots (never)
    if (sw.pr_debug)
        std::fprintf(stderr, "prk: large objects %u, chunked: taken %u done %u failed %u; chunks %u, walked again %u\n",
                     nbig, walks.npr, S.h_rb[4], S.h_rb[5], walks.pr_chunks, S.h_rb[6]);
    c->stats.objects_chunked += S.h_rb[4];
    c->stats.objects_walked += nbig - S.h_rb[4];
    c->stats.object_chunks += walks.pr_chunks;
    c->stats.object_chunks_rewalked += S.h_rb[6];
    c->stats.triangles = T;
    c->stats.tiles = ntiles;
    c->stats.bin_entries = total;
    PRK_TRY(S.d_vals_b.ensure((size_t)std::max<uint32_t>(total, 1) * 4));
    PRK_TRY(prk_span_bin(&fp, S.d_pos.as<SpanPos>(), nslot, toff, tcnt, (uint32_t *)S.d_vals_b.p, s));
    PRK_TRY(S.d_nwin.ensure((size_t)ntiles * 4));
    PRK_TRY(S.d_wtag.ensure((size_t)ntiles * fp.tile_w * fp.tile_h * 4));
    PRK_TRY(prk_launch_spans(&fp, (const uint32_t *)S.d_offs.p, (const uint32_t *)S.d_vals_b.p, S.d_pos.as<SpanPos>(),
                             S.d_recs.as<SpanRec>(), srecs(), modes, (const uint32_t *)S.d_span_tri.p,
                             (uint32_t *)S.d_nwin.p, (uint32_t *)S.d_wtag.p, s));
    return PRK_OK;
}
}  // namespace

// One pass of whole-object AETs (prk_spans.hip): FillEdgeTable per triangle,
// MergeSort per object (one radix sort), one walk of every object's AET into
// span records (each object writing into its own slots, as many as its edges'
// active rows allow), bin the spans to tiles, then visibility + shading.
// Stream-ordered on s; the host waits at the two sizes it reads back (the
// span slots in sizes(), the bin entry count in bin_shade()).
int flush_spans(prk_context *c, hipStream_t s, const std::vector<prk::DrawRec> &draws, uint32_t T,
                       uint32_t win_base) {
    c->z_early = false;  // (k_pix / k_span_shade write a span pass's z)
    const bool fuse = c->clear_pending && T > 0;
    SpanPass P(c, s, draws);
    frame_params(c, P.fp);
    P.fp.tri_count = T;
    P.fp.ndraws = (uint32_t)draws.size();
    P.fp.win_base = win_base;
    P.ntiles = (uint32_t)(P.fp.tiles_x * P.fp.tiles_y);
    c->clear_pending = false;
    P.fp.clear_fused = fuse ? 1 : 0;
    if (T == 0) return PRK_OK;
    if (!P.S.h_rb) PRK_TRY(hipHostMalloc((void **)&P.S.h_rb, 8 * sizeof(uint32_t), hipHostMallocDefault));
    P.lcap = prk_obj_walk_lcap();
    int rc = P.plan();
    if (rc == PRK_OK) rc = P.upload();
    if (rc == PRK_OK) rc = P.edges();
    if (rc == PRK_OK) rc = P.sizes();
    if (rc != PRK_OK) return rc;
    P.classify();
    rc = P.walk();
    if (rc == PRK_OK) rc = P.bin_shade(T);
    return rc;
}

int prk_debug_stage_bytes(prk_context *c, uint64_t *bytes_out) {
    if (!c || !bytes_out) return PRK_ERR_ARG;
    *bytes_out = c->spans.last_stage_bytes;
    return PRK_OK;
}

int prk_debug_walk_routes(prk_context *c, uint32_t *out, int32_t n) {
    if (!c || !out || n < 0 || n > 12) return PRK_ERR_ARG;
    RESOLVE_COUNT(c);
    const prk_context::SpanScratch &S = c->spans;
    for (int i = 0; i < n; ++i) out[i] = i < 9 ? S.walk_routes[i] : (uint32_t)S.walk_sizes[i - 9];
    return PRK_OK;
}

}  // extern "C"
