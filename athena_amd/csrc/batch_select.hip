// Mini-batches out of a device-resident dataset graph (athena_mp_batch_plan_create / athena_mp_batch_select; the definition is in
// include/athena_mp.h).  The dataset handle is block-diagonal: a structure's rows, its transposed rows and its edge columns are
// three contiguous ranges of the handle's arrays, so a batch is a concatenation of slices with three kinds of index rebased.  The
// plan checks that once, on the device, and keeps per-structure tables; a select then computes every size and every base on the
// host, uploads one small table and copies all thirteen arrays and both maps in ONE launch.  No sort, no neighbour search, no
// device -> host copy and no atomics: two selects of the same ids are byte-identical.
#include <string.h>

#include <algorithm>
#include <vector>

#include "common.h"

namespace {

constexpr int kChunk = 4096;        // elements of one array a wave copies for one item: a hub row and a 130 k-structure batch both balance
constexpr int kCheckEntries = 4096; // entries of one work item of the check (at least one row)
constexpr int kWavesPerBlock = 4;
constexpr int kMaxBlocks = 4096;

struct CheckItem {
    int32_t s, r0, r1;   // structure, rows [r0, r1)
};
struct CheckSlot {
    int32_t flag, band, max_row, max_col;
};

inline __device__ int32_t wave_max(int32_t v)
{
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    return v;
}

// One wave per item, one row per lane at a time: every entry of the rows [r0, r1) of structure s must stay inside the structure.
// The item's findings go to its own slot with plain stores; the host folds the slots.
__global__ __launch_bounds__(64 * kWavesPerBlock) void batch_check_kernel(const CheckItem *items, int32_t n_items, const int32_t *rowptr,
                                                                          const int32_t *col, const int32_t *eid, const int32_t *t_rowptr,
                                                                          const int32_t *off, const int32_t *eoff, CheckSlot *slots)
{
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    for (int64_t it = (int64_t)blockIdx.x * kWavesPerBlock + wave; it < n_items; it += (int64_t)gridDim.x * kWavesPerBlock) {
        const CheckItem c = items[it];
        const int32_t lo = off[c.s], hi = off[c.s + 1];
        const int32_t elo = eoff ? eoff[c.s] : 0, ehi = eoff ? eoff[c.s + 1] : 0;
        int32_t flag = 0, band = 0, mrow = 0, mcol = 0;
        for (int32_t r = c.r0 + lane; r < c.r1; r += 64) {
            const int32_t b = rowptr[r], e = rowptr[r + 1];
            mrow = max(mrow, e - b);
            mcol = max(mcol, t_rowptr[r + 1] - t_rowptr[r]);
            for (int32_t k = b; k < e; ++k) {
                const int32_t u = col[k], id = eid[k];
                if (u < lo || u >= hi) flag = 1;
                if (id < -1 || (id >= 0 && (id < elo || id >= ehi))) flag = 1;
                const int32_t d = u - r;
                band = max(band, d < 0 ? -d : d);
            }
        }
        flag = wave_max(flag);
        band = wave_max(band);
        mrow = wave_max(mrow);
        mcol = wave_max(mcol);
        if (lane == 0) slots[it] = CheckSlot{flag, band, mrow, mcol};
    }
}

// what a select copies from and to, and the tables that say where
struct CopyArgs {
    // parent / child arrays, in the order of athena_mp_graph_export
    const int32_t *p_rowptr, *p_col, *p_eid, *p_coef, *p_t_rowptr, *p_t_src, *p_t_eid, *p_t_coef, *p_e_rowptr, *p_e_row, *p_e_col,
        *p_deg_row, *p_deg_col;
    int32_t *c_rowptr, *c_col, *c_eid, *c_coef, *c_t_rowptr, *c_t_src, *c_t_eid, *c_t_coef, *c_e_rowptr, *c_e_row, *c_e_col, *c_deg_row,
        *c_deg_col;
    int32_t *vertex_map, *edge_map;   // each may be null
    // per structure [B + 1], resident with the plan: first vertex, first entry, first edge column, first entry of the edge index
    const int32_t *off, *wst, *eoff, *est;
    // per selected slot [m], uploaded by the select: the structure and where it lands in the child
    const int32_t *sel, *cv, *cw, *ce, *cq;
    const int32_t *items;   // [n_items][2] = (slot t, part p): elements [p * kChunk, (p + 1) * kChunk) of each of the slot's arrays
    int32_t n_items;
    int32_t n_child, nnz_child, ne_child, nq_child;   // the closing elements of the three row pointers
};

enum { kRaw = 0, kAdd = 1, kAddKeep = 2, kIota = 3 };

// elements [p * kChunk, ...) of an n-element slice: dst[db + i] = f(src[sb + i]); 64 elements per step, 4-byte accesses (a slice
// starts at an arbitrary element of its array)
template <int MODE>
inline __device__ void copy_part(int32_t *dst, const int32_t *src, int32_t db, int32_t sb, int32_t n, int32_t p, int32_t add, int lane)
{
    const int32_t b = p * kChunk, e = min(n, b + kChunk);
    for (int32_t i = b + lane; i < e; i += 64) {
        int32_t v;
        if (MODE == kIota) {
            v = sb + i;
        } else {
            v = src[sb + i];
            if (MODE == kAdd) v += add;
            if (MODE == kAddKeep) v = v < 0 ? -1 : v + add;
        }
        dst[db + i] = v;
    }
}

__global__ __launch_bounds__(64 * kWavesPerBlock) void batch_copy_kernel(const CopyArgs a)
{
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    for (int64_t it = (int64_t)blockIdx.x * kWavesPerBlock + wave; it < a.n_items; it += (int64_t)gridDim.x * kWavesPerBlock) {
        const int32_t t = a.items[2 * it], p = a.items[2 * it + 1];
        const int32_t s = a.sel[t];
        const int32_t v0 = a.off[s], nv = a.off[s + 1] - v0;
        const int32_t w0 = a.wst[s], nw = a.wst[s + 1] - w0;
        const int32_t e0 = a.eoff[s], ne = a.eoff[s + 1] - e0;
        const int32_t q0 = a.est[s], nq = a.est[s + 1] - q0;
        const int32_t cv = a.cv[t], cw = a.cw[t], ce = a.ce[t], cq = a.cq[t];
        const int32_t dv = cv - v0, dw = cw - w0, de = ce - e0;
        // forward CSR
        copy_part<kAdd>(a.c_rowptr, a.p_rowptr, cv, v0, nv, p, dw, lane);
        copy_part<kAdd>(a.c_col, a.p_col, cw, w0, nw, p, dv, lane);
        copy_part<kAddKeep>(a.c_eid, a.p_eid, cw, w0, nw, p, de, lane);
        copy_part<kRaw>(a.c_coef, a.p_coef, cw, w0, nw, p, 0, lane);
        // transposed CSR: cut at the same vertices, and (checked by the plan) at the same entries
        copy_part<kAdd>(a.c_t_rowptr, a.p_t_rowptr, cv, v0, nv, p, dw, lane);
        copy_part<kAdd>(a.c_t_src, a.p_t_src, cw, w0, nw, p, dv, lane);
        copy_part<kAddKeep>(a.c_t_eid, a.p_t_eid, cw, w0, nw, p, de, lane);
        copy_part<kRaw>(a.c_t_coef, a.p_t_coef, cw, w0, nw, p, 0, lane);
        // edge-column index
        copy_part<kAdd>(a.c_e_rowptr, a.p_e_rowptr, ce, e0, ne, p, cq - q0, lane);
        copy_part<kAdd>(a.c_e_row, a.p_e_row, cq, q0, nq, p, dv, lane);
        copy_part<kAdd>(a.c_e_col, a.p_e_col, cq, q0, nq, p, dw, lane);
        copy_part<kRaw>(a.c_deg_row, a.p_deg_row, cv, v0, nv, p, 0, lane);
        copy_part<kRaw>(a.c_deg_col, a.p_deg_col, cv, v0, nv, p, 0, lane);
        if (a.vertex_map) copy_part<kIota>(a.vertex_map, nullptr, cv, v0, nv, p, 0, lane);
        if (a.edge_map) copy_part<kIota>(a.edge_map, nullptr, ce, e0, ne, p, 0, lane);
        if (it == 0 && lane == 0) {   // item 0 always exists (n_sel >= 1)
            a.c_rowptr[a.n_child] = a.nnz_child;
            a.c_t_rowptr[a.n_child] = a.nnz_child;
            a.c_e_rowptr[a.ne_child] = a.nq_child;
        }
    }
}

struct LongRow {
    int32_t row, beg, len;   // all relative to the structure: row, first entry, entries
};

int grid_for(int64_t n_items)
{
    return (int)std::max<int64_t>(1, std::min<int64_t>((n_items + kWavesPerBlock - 1) / kWavesPerBlock, kMaxBlocks));
}

}   // namespace

struct athena_mp_batch_plan {
    const athena_mp_graph *g = nullptr;
    int32_t B = 0;
    bool has_edges = false;
    // per structure [B + 1] on the host: first vertex, first entry (forward = transposed), first edge column, first entry of the edge index
    std::vector<int32_t> off, wst, eoff, est;
    std::vector<int32_t> band, max_row, max_col;   // [B]
    std::vector<int32_t> lf0, lb0;                 // [B + 1] first long row of each structure in lf / lb
    std::vector<LongRow> lf, lb;                   // rows longer than kLongRow of the forward / transposed CSR
    int32_t *d_tab = nullptr;                      // off | wst | eoff | est, [4][B + 1] in HBM
    // pinned staging of a select's tables; `staged` says when the stream has taken the previous select's copy
    mutable void *h_stage = nullptr;
    mutable size_t h_stage_bytes = 0;
    mutable hipEvent_t staged = nullptr;
    mutable bool staged_pending = false;
};

static int plan_free(athena_mp_batch_plan *p)
{
    if (p->staged) {
        if (p->staged_pending) (void)hipEventSynchronize(p->staged);
        (void)hipEventDestroy(p->staged);
    }
    if (p->h_stage) (void)hipHostFree(p->h_stage);
    if (p->d_tab) (void)hipFree(p->d_tab);
    delete p;
    return 0;
}

static void long_rows(const std::vector<int32_t> &rp, const std::vector<int32_t> &off, int32_t B, std::vector<int32_t> *first,
                      std::vector<LongRow> *rows)
{
    first->assign((size_t)B + 1, 0);
    for (int32_t s = 0; s < B; ++s) {
        (*first)[s] = (int32_t)rows->size();
        for (int32_t r = off[s]; r < off[s + 1]; ++r)
            if (rp[r + 1] - rp[r] > kLongRow) rows->push_back(LongRow{r - off[s], rp[r] - rp[off[s]], rp[r + 1] - rp[r]});
    }
    (*first)[B] = (int32_t)rows->size();
}

extern "C" {

int athena_mp_batch_plan_destroy(athena_mp_batch_plan *p)
{
    if (!p) return 0;
    return plan_free(p);
}

int athena_mp_batch_plan_create(const athena_mp_graph *g, int32_t n_structures, const int32_t *offsets, const int64_t *edge_offsets,
                                athena_mp_batch_plan **out)
{
    AMP_REQUIRE(out != nullptr, "batch_plan_create: null out pointer");
    *out = nullptr;
    AMP_REQUIRE(g != nullptr && offsets != nullptr, "batch_plan_create: null argument");
    AMP_REQUIRE(n_structures >= 0, "batch_plan_create: n_structures = %d", n_structures);
    AMP_REQUIRE(g->n_rows == g->n_cols, "batch_plan_create: a rectangular handle (%d x %d) is a shard block, not a dataset", g->n_rows,
                g->n_cols);
    const int32_t B = n_structures, n = g->n_rows;
    AMP_REQUIRE(edge_offsets == nullptr || g->n_edge_cols > 0 || edge_offsets[B] == 0,
                "batch_plan_create: edge_offsets given, the handle has no edge columns");
    AMP_REQUIRE(edge_offsets != nullptr || g->n_edge_cols == 0, "batch_plan_create: the handle has %d edge columns and edge_offsets is null",
                g->n_edge_cols);
    AMP_REQUIRE(offsets[0] == 0, "batch_plan_create: offsets(1) = %d, not 0", offsets[0]);
    for (int32_t s = 0; s < B; ++s)
        AMP_REQUIRE(offsets[s + 1] >= offsets[s], "batch_plan_create: structure %d: offsets descend from %d to %d", s + 1, offsets[s],
                    offsets[s + 1]);
    AMP_REQUIRE(offsets[B] == n, "batch_plan_create: offsets end at %d, the handle has %d rows", offsets[B], n);
    const bool has_edges = edge_offsets != nullptr && g->n_edge_cols > 0;
    if (edge_offsets) {
        AMP_REQUIRE(edge_offsets[0] == 0, "batch_plan_create: edge_offsets(1) = %lld, not 0", (long long)edge_offsets[0]);
        for (int32_t s = 0; s < B; ++s)
            AMP_REQUIRE(edge_offsets[s + 1] >= edge_offsets[s], "batch_plan_create: structure %d: edge_offsets descend from %lld to %lld",
                        s + 1, (long long)edge_offsets[s], (long long)edge_offsets[s + 1]);
        AMP_REQUIRE(edge_offsets[B] == (int64_t)g->n_edge_cols, "batch_plan_create: edge_offsets end at %lld, the handle has %d edge columns",
                    (long long)edge_offsets[B], g->n_edge_cols);
    }

    // the three row pointers on the host, once: every table of the plan comes from them
    std::vector<int32_t> rp((size_t)n + 1), trp((size_t)n + 1), erp((size_t)g->n_edge_cols + 1);
    AMP_HIP(hipMemcpyAsync(rp.data(), g->rowptr, sizeof(int32_t) * rp.size(), hipMemcpyDeviceToHost, amp::stream()));
    AMP_HIP(hipMemcpyAsync(trp.data(), g->t_rowptr, sizeof(int32_t) * trp.size(), hipMemcpyDeviceToHost, amp::stream()));
    AMP_HIP(hipMemcpyAsync(erp.data(), g->e_rowptr, sizeof(int32_t) * erp.size(), hipMemcpyDeviceToHost, amp::stream()));
    AMP_HIP(hipStreamSynchronize(amp::stream()));
    for (int32_t r = 0; r < n; ++r) {
        const int32_t deg = (size_t)r < g->h_deg_row.size() ? g->h_deg_row[r] : -1;
        AMP_REQUIRE(deg == rp[r + 1] - rp[r], "batch_plan_create: row %d has %d entries and degree %d: a handle with explicit degrees", r + 1,
                    rp[r + 1] - rp[r], deg);
    }

    athena_mp_batch_plan *p = new athena_mp_batch_plan();
    p->g = g;
    p->B = B;
    p->has_edges = has_edges;
    p->off.assign(offsets, offsets + B + 1);
    p->wst.resize((size_t)B + 1);
    p->eoff.assign((size_t)B + 1, 0);
    p->est.assign((size_t)B + 1, 0);
    for (int32_t s = 0; s <= B; ++s) {
        p->wst[s] = rp[offsets[s]];
        if (has_edges) {
            p->eoff[s] = (int32_t)edge_offsets[s];
            p->est[s] = erp[edge_offsets[s]];
        }
        if (trp[offsets[s]] != rp[offsets[s]]) {
            amp::set_error("batch_plan_create: structure %d: %d forward entries before it, %d transposed ones: an entry leaves its structure",
                           std::min(s + 1, B), rp[offsets[s]], trp[offsets[s]]);
            plan_free(p);
            return 2;
        }
    }

    // the block-diagonal condition, entry by entry, on the device
    std::vector<CheckItem> items;
    for (int32_t s = 0; s < B; ++s) {
        int32_t r0 = offsets[s];
        while (r0 < offsets[s + 1]) {
            int32_t r1 = r0 + 1;
            while (r1 < offsets[s + 1] && rp[r1 + 1] - rp[r0] <= kCheckEntries && r1 - r0 < 64 * 64) ++r1;
            items.push_back(CheckItem{s, r0, r1});
            r0 = r1;
        }
    }
    p->band.assign((size_t)B, 0);
    p->max_row.assign((size_t)B, 0);
    p->max_col.assign((size_t)B, 0);
    int rc = 0;
    {
        amp::Scratch scratch;
        CheckItem *d_items = nullptr;
        CheckSlot *d_slots = nullptr;
        const size_t tab = (size_t)B + 1;
        std::vector<int32_t> h_tab(4 * tab);
        memcpy(h_tab.data(), p->off.data(), 4 * tab);
        memcpy(h_tab.data() + tab, p->wst.data(), 4 * tab);
        memcpy(h_tab.data() + 2 * tab, p->eoff.data(), 4 * tab);
        memcpy(h_tab.data() + 3 * tab, p->est.data(), 4 * tab);
        std::vector<CheckSlot> slots(items.size());
        auto body = [&]() -> int {
            AMP_HIP(hipMalloc((void **)&p->d_tab, sizeof(int32_t) * h_tab.size()));
            AMP_HIP(hipMemcpyAsync(p->d_tab, h_tab.data(), sizeof(int32_t) * h_tab.size(), hipMemcpyHostToDevice, amp::stream()));
            if (!items.empty()) {
                if (scratch.get(&d_items, items.size()) || scratch.get(&d_slots, items.size())) return 1;
                AMP_HIP(hipMemcpyAsync(d_items, items.data(), sizeof(CheckItem) * items.size(), hipMemcpyHostToDevice, amp::stream()));
                hipLaunchKernelGGL(batch_check_kernel, dim3(grid_for((int64_t)items.size())), dim3(64 * kWavesPerBlock), 0, amp::stream(),
                                   d_items, (int32_t)items.size(), g->rowptr, g->col, g->eid, g->t_rowptr, p->d_tab,
                                   has_edges ? p->d_tab + 2 * tab : nullptr, d_slots);
                AMP_LAUNCH_CHECK();
                AMP_HIP(hipMemcpyAsync(slots.data(), d_slots, sizeof(CheckSlot) * slots.size(), hipMemcpyDeviceToHost, amp::stream()));
            }
            AMP_HIP(hipStreamSynchronize(amp::stream()));
            AMP_HIP(hipEventCreateWithFlags(&p->staged, hipEventDisableTiming));
            return 0;
        };
        rc = body();
        for (size_t i = 0; rc == 0 && i < items.size(); ++i) {
            const int32_t s = items[i].s;
            if (slots[i].flag) {
                amp::set_error("batch_plan_create: structure %d (rows %d..%d): an entry leaves its structure (a neighbour outside its rows, or an "
                               "edge column outside its edge columns)", s + 1, offsets[s] + 1, offsets[s + 1]);
                rc = 2;
                break;
            }
            p->band[s] = std::max(p->band[s], slots[i].band);
            p->max_row[s] = std::max(p->max_row[s], slots[i].max_row);
            p->max_col[s] = std::max(p->max_col[s], slots[i].max_col);
        }
    }
    if (rc) {
        plan_free(p);
        return rc;
    }
    long_rows(rp, p->off, B, &p->lf0, &p->lf);
    long_rows(trp, p->off, B, &p->lb0, &p->lb);
    *out = p;
    return 0;
}

int athena_mp_batch_select(const athena_mp_batch_plan *p, int32_t n_sel, const int32_t *sel, athena_mp_graph **out, int32_t *offsets_out,
                           int64_t *edge_offsets_out, int32_t *vertex_map, int32_t *edge_map)
{
    if (out) *out = nullptr;
    AMP_REQUIRE(p != nullptr, "batch_select: null argument");
    AMP_REQUIRE(n_sel >= 1, "batch_select: n_sel = %d, need at least one structure", n_sel);
    AMP_REQUIRE(sel != nullptr, "batch_select: null argument");
    const int32_t m = n_sel, B = p->B;
    // every size and every base of the child, on the host
    std::vector<int32_t> tab(5 * (size_t)m);   // sel | cv | cw | ce | cq
    int32_t *t_sel = tab.data(), *t_cv = t_sel + m, *t_cw = t_cv + m, *t_ce = t_cw + m, *t_cq = t_ce + m;
    int64_t nv = 0, nw = 0, ne = 0, nq = 0, n_items = 0, n_lf = 0, n_lb = 0;
    int32_t max_row = 0, max_col = 0, band = 0;
    for (int32_t t = 0; t < m; ++t) {
        const int32_t s = sel[t];
        AMP_REQUIRE(s >= 0 && s < B, "batch_select: id %d at position %d is outside [0, %d)", s, t, B);
        t_sel[t] = s;
        t_cv[t] = (int32_t)nv;
        t_cw[t] = (int32_t)nw;
        t_ce[t] = (int32_t)ne;
        t_cq[t] = (int32_t)nq;
        if (offsets_out) offsets_out[t] = (int32_t)nv;
        if (edge_offsets_out) edge_offsets_out[t] = ne;
        const int64_t sv = p->off[s + 1] - p->off[s], sw = p->wst[s + 1] - p->wst[s];
        nv += sv;
        nw += sw;
        ne += p->eoff[s + 1] - p->eoff[s];
        nq += p->est[s + 1] - p->est[s];
        AMP_REQUIRE(nw < (int64_t)INT32_MAX && nv < (int64_t)INT32_MAX, "batch_select: the batch has 2^31 entries or more at position %d (id %d)",
                    t, s);
        n_items += std::max<int64_t>(1, (std::max({sv, sw, (int64_t)(p->eoff[s + 1] - p->eoff[s])}) + kChunk - 1) / kChunk);
        max_row = std::max(max_row, p->max_row[s]);
        max_col = std::max(max_col, p->max_col[s]);
        band = std::max(band, p->band[s]);
        n_lf += p->lf0[s + 1] - p->lf0[s];
        n_lb += p->lb0[s + 1] - p->lb0[s];
    }
    AMP_REQUIRE(n_items < (int64_t)INT32_MAX, "batch_select: %lld work items", (long long)n_items);
    if (offsets_out) offsets_out[m] = (int32_t)nv;
    if (edge_offsets_out) edge_offsets_out[m] = ne;
    if (out == nullptr) return 0;   // size query: the device is not touched

    // long-row plans of the child, from the plan's lists
    std::vector<int32_t> lp[2][4];   // [fwd / bwd][task_beg, task_end, row_id, row_task0]
    for (int dir = 0; dir < 2; ++dir) {
        const std::vector<int32_t> &first = dir ? p->lb0 : p->lf0;
        const std::vector<LongRow> &rows = dir ? p->lb : p->lf;
        if ((dir ? n_lb : n_lf) == 0) continue;
        for (int32_t t = 0; t < m; ++t) {
            const int32_t s = sel[t];
            for (int32_t k = first[s]; k < first[s + 1]; ++k) {
                const int32_t beg = t_cw[t] + rows[k].beg, end = beg + rows[k].len;
                lp[dir][2].push_back(t_cv[t] + rows[k].row);
                lp[dir][3].push_back((int32_t)lp[dir][0].size());
                for (int32_t b = beg; b < end; b += kLongRow) {
                    lp[dir][0].push_back(b);
                    lp[dir][1].push_back(std::min(b + kLongRow, end));
                }
            }
        }
        lp[dir][3].push_back((int32_t)lp[dir][0].size());
    }

    // one pinned staging block: the slot tables, the items, the long-row plans
    size_t stage_ints = tab.size() + 2 * (size_t)n_items;
    for (int dir = 0; dir < 2; ++dir)
        for (int k = 0; k < 4; ++k) stage_ints += lp[dir][k].size();
    if (p->staged_pending) {   // the stream may still be reading the previous select's tables out of the staging block
        AMP_HIP(hipEventSynchronize(p->staged));
        p->staged_pending = false;
    }
    if (p->h_stage_bytes < sizeof(int32_t) * stage_ints) {
        if (p->h_stage) AMP_HIP(hipHostFree(p->h_stage));
        p->h_stage = nullptr;
        p->h_stage_bytes = 0;
        const size_t want = sizeof(int32_t) * (stage_ints + (stage_ints >> 2)) + 256;
        AMP_HIP(hipHostMalloc(&p->h_stage, want, hipHostMallocDefault));
        p->h_stage_bytes = want;
    }
    int32_t *h = (int32_t *)p->h_stage;
    memcpy(h, tab.data(), sizeof(int32_t) * tab.size());
    int32_t *h_items = h + tab.size();
    {
        int64_t i = 0;
        for (int32_t t = 0; t < m; ++t) {
            const int32_t s = sel[t];
            const int64_t big = std::max({(int64_t)(p->off[s + 1] - p->off[s]), (int64_t)(p->wst[s + 1] - p->wst[s]), (int64_t)(p->eoff[s + 1] - p->eoff[s])});
            const int32_t parts = (int32_t)std::max<int64_t>(1, (big + kChunk - 1) / kChunk);
            for (int32_t q = 0; q < parts; ++q, ++i) {
                h_items[2 * i] = t;
                h_items[2 * i + 1] = q;
            }
        }
    }
    int32_t *h_lp = h_items + 2 * n_items;

    athena_mp_graph *c = new athena_mp_graph();
    const athena_mp_graph *g = p->g;
    c->n_rows = c->n_cols = (int32_t)nv;
    c->nnz = nw;
    c->n_edge_cols = (int32_t)ne;
    c->n_with_edge = nq;
    c->max_row_len = max_row;
    c->max_col_len = max_col;
    c->band = band > 64 ? INT32_MAX : band;
    c->h_deg_row.resize((size_t)nv);
    for (int32_t t = 0; t < m; ++t) {
        const int32_t s = sel[t], cnt = p->off[s + 1] - p->off[s];
        if (cnt > 0) memcpy(c->h_deg_row.data() + t_cv[t], g->h_deg_row.data() + p->off[s], sizeof(int32_t) * (size_t)cnt);
    }
    auto body = [&]() -> int {
        auto alloc = [](void **ptr, int64_t count) { return hipMalloc(ptr, sizeof(int32_t) * (size_t)(count > 0 ? count : 1)); };
        AMP_HIP(alloc((void **)&c->rowptr, nv + 1));
        AMP_HIP(alloc((void **)&c->col, nw));
        AMP_HIP(alloc((void **)&c->eid, nw));
        AMP_HIP(alloc((void **)&c->coef, nw));
        AMP_HIP(alloc((void **)&c->t_rowptr, nv + 1));
        AMP_HIP(alloc((void **)&c->t_src, nw));
        AMP_HIP(alloc((void **)&c->t_eid, nw));
        AMP_HIP(alloc((void **)&c->t_coef, nw));
        AMP_HIP(alloc((void **)&c->e_rowptr, ne + 1));
        AMP_HIP(alloc((void **)&c->e_row, nq));
        AMP_HIP(alloc((void **)&c->e_col, nq));
        AMP_HIP(alloc((void **)&c->deg_row, nv));
        AMP_HIP(alloc((void **)&c->deg_col, nv));
        for (int dir = 0; dir < 2; ++dir) {
            LongPlan *l = dir ? &c->lp_bwd : &c->lp_fwd;
            l->n_tasks = (int32_t)lp[dir][0].size();
            l->n_long = (int32_t)lp[dir][2].size();
            if (l->n_long == 0) continue;
            int32_t **dst[4] = {&l->task_beg, &l->task_end, &l->row_id, &l->row_task0};
            for (int k = 0; k < 4; ++k) {
                const size_t bytes = sizeof(int32_t) * lp[dir][k].size();
                memcpy(h_lp, lp[dir][k].data(), bytes);
                AMP_HIP(hipMalloc((void **)dst[k], bytes));
                AMP_HIP(hipMemcpyAsync(*dst[k], h_lp, bytes, hipMemcpyHostToDevice, amp::stream()));
                h_lp += lp[dir][k].size();
            }
        }
        void *d_stage = nullptr;
        const size_t up_ints = tab.size() + 2 * (size_t)n_items;
        if (amp::named_buffer("batch.select", sizeof(int32_t) * (up_ints + (up_ints >> 2)), false, &d_stage)) return 1;
        AMP_HIP(hipMemcpyAsync(d_stage, h, sizeof(int32_t) * up_ints, hipMemcpyHostToDevice, amp::stream()));
        const int32_t *d = (const int32_t *)d_stage;
        const size_t tb = (size_t)B + 1;
        CopyArgs a;
        a.p_rowptr = g->rowptr; a.p_col = g->col; a.p_eid = g->eid; a.p_coef = (const int32_t *)g->coef;
        a.p_t_rowptr = g->t_rowptr; a.p_t_src = g->t_src; a.p_t_eid = g->t_eid; a.p_t_coef = (const int32_t *)g->t_coef;
        a.p_e_rowptr = g->e_rowptr; a.p_e_row = g->e_row; a.p_e_col = g->e_col; a.p_deg_row = g->deg_row; a.p_deg_col = g->deg_col;
        a.c_rowptr = c->rowptr; a.c_col = c->col; a.c_eid = c->eid; a.c_coef = (int32_t *)c->coef;
        a.c_t_rowptr = c->t_rowptr; a.c_t_src = c->t_src; a.c_t_eid = c->t_eid; a.c_t_coef = (int32_t *)c->t_coef;
        a.c_e_rowptr = c->e_rowptr; a.c_e_row = c->e_row; a.c_e_col = c->e_col; a.c_deg_row = c->deg_row; a.c_deg_col = c->deg_col;
        a.vertex_map = vertex_map;
        a.edge_map = edge_map;
        a.off = p->d_tab; a.wst = p->d_tab + tb; a.eoff = p->d_tab + 2 * tb; a.est = p->d_tab + 3 * tb;
        a.sel = d; a.cv = d + m; a.cw = d + 2 * (size_t)m; a.ce = d + 3 * (size_t)m; a.cq = d + 4 * (size_t)m;
        a.items = d + 5 * (size_t)m;
        a.n_items = (int32_t)n_items;
        a.n_child = (int32_t)nv; a.nnz_child = (int32_t)nw; a.ne_child = (int32_t)ne; a.nq_child = (int32_t)nq;
        hipLaunchKernelGGL(batch_copy_kernel, dim3(grid_for(n_items)), dim3(64 * kWavesPerBlock), 0, amp::stream(), a);
        AMP_LAUNCH_CHECK();
        AMP_HIP(hipEventRecord(p->staged, amp::stream()));
        p->staged_pending = true;
        return 0;
    };
    const int rc = body();
    if (rc) {
        (void)hipStreamSynchronize(amp::stream());   // copies out of the staging block may be in flight
        p->staged_pending = false;
        athena_mp_graph_destroy(c);
        return rc;
    }
    *out = c;
    return 0;
}

}   // extern "C"
