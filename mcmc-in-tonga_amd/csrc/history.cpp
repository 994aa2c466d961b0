// history.cpp -- td_history behind the C ABI: allocation, counts, the bulk
// read, and the host engines' append.  The DEVICE engine's samples are written
// by k_chain_run itself (chain_kernels.hip record_sample).
#include "history.h"

#include "../../include/tdstar_testing.h"

#include <algorithm>
#include <new>
#include <string>

using namespace tdstar;

namespace {

template <class T>
T *carve(char *&cur, size_t count) {
    T *p = reinterpret_cast<T *>(cur);
    cur += ((count * sizeof(T) + 255) / 256) * 256;
    return p;
}

size_t padded(size_t bytes) { return ((bytes + 255) / 256) * 256; }

}  // namespace

namespace tdstar {

int history_check_room(const td_history *h, int64_t added, int64_t cells_each, const char *who) {
    if (h->samples + added > h->max_samples)
        return set_err(h->ctx, TD_ERR_ARG,
                       std::string(who) + ": the history has room for " + std::to_string(h->max_samples - h->samples) +
                           " more samples, the run takes " + std::to_string(added));
    const int64_t used = h->off[(size_t)h->samples];
    if (added > 0 && cells_each > (h->max_cells - used) / added)
        return set_err(h->ctx, TD_ERR_ARG,
                       std::string(who) + ": the history has room for " + std::to_string(h->max_cells - used) +
                           " more cells, the run may take " + std::to_string(added) + " x " +
                           std::to_string(cells_each));
    return TD_OK;
}

int history_adopt(td_history *h, int64_t added) {
    if (added <= 0) return TD_OK;
    h->off.resize((size_t)(h->samples + added + 1));
    TD_HIP(h->ctx, hipMemcpy(h->off.data() + h->samples + 1, h->d.off + h->samples + 1,
                             sizeof(int64_t) * (size_t)added, hipMemcpyDeviceToHost));
    h->samples += added;
    return TD_OK;
}

int history_pack_adopt(td_history *h, int64_t added, int64_t cells_each) {
    if (added <= 0) return TD_OK;
    td_ctx *c = h->ctx;
    const int64_t base = h->samples, used = h->off[(size_t)base];
    Timer *tm = c->timer.on ? &c->timer : nullptr;
    hipEvent_t t0 = tm ? tm->begin(c->stream) : nullptr;
    const hipError_t e = launch_history_pack(h->d.cells, h->d.stride, (long long)used, (long long)cells_each,
                                             h->d.ncells + base, (long long)added, h->d.off + base, c->stream);
    if (tm) tm->end("history_pack", t0, c->stream);
    if (e != hipSuccess) return hip_err(c, e, "k_history_pack launch");
    TD_HIP(c, hipStreamSynchronize(c->stream));
    return history_adopt(h, added);
}

int history_append_host(td_history *h, const double *x, const double *y, const double *z, const double *zeta,
                        int64_t ncells, double phi, int64_t iter, int action, int accept, const double *ptS) {
    td_ctx *c = h->ctx;
    const int64_t k = h->samples, o = h->off[(size_t)k];
    if (k >= h->max_samples || ncells > h->max_cells - o)
        return set_err(c, TD_ERR_ARG, "history append: no room");  // (the callers check before they run)
    const double *src[4] = {x, y, z, zeta};
    for (int comp = 0; comp < 4 && ncells > 0; ++comp)
        TD_HIP(c, hipMemcpy(h->d.cells + comp * h->d.stride + o, src[comp], sizeof(double) * (size_t)ncells,
                            hipMemcpyHostToDevice));
    const long long it = iter, o1 = o + ncells;
    const int nc = (int)ncells;
    TD_HIP(c, hipMemcpy(h->d.iter + k, &it, sizeof(it), hipMemcpyHostToDevice));
    TD_HIP(c, hipMemcpy(h->d.phi + k, &phi, sizeof(phi), hipMemcpyHostToDevice));
    TD_HIP(c, hipMemcpy(h->d.ncells + k, &nc, sizeof(nc), hipMemcpyHostToDevice));
    TD_HIP(c, hipMemcpy(h->d.action + k, &action, sizeof(action), hipMemcpyHostToDevice));
    TD_HIP(c, hipMemcpy(h->d.accept + k, &accept, sizeof(accept), hipMemcpyHostToDevice));
    TD_HIP(c, hipMemcpy(h->d.off + k + 1, &o1, sizeof(o1), hipMemcpyHostToDevice));
    if (h->d.ptS && h->n > 0 && ptS)
        TD_HIP(c, hipMemcpy(h->d.ptS + k * h->n, ptS, sizeof(double) * (size_t)h->n, hipMemcpyHostToDevice));
    h->off.push_back(o1);
    h->samples = k + 1;
    return TD_OK;
}

}  // namespace tdstar

extern "C" {

int td_history_create(td_history **out, td_ctx *ctx, int64_t max_samples, int64_t max_cells_total, int with_ptS) {
    // (every check before any HIP call)
    if (out) *out = nullptr;
    if (max_samples < 1) return set_err(ctx, TD_ERR_ARG, "td_history_create: need max_samples >= 1");
    if (max_cells_total < 1) return set_err(ctx, TD_ERR_ARG, "td_history_create: need max_cells_total >= 1");
    if (!ctx) return set_err(nullptr, TD_ERR_ARG, "td_history_create: ctx is NULL");
    if (!out) return set_err(ctx, TD_ERR_ARG, "td_history_create: out is NULL");
    const int64_t n = ctx->g.n;
    if (max_samples > ((int64_t)1 << 40) || max_cells_total > ((int64_t)1 << 40) ||
        (with_ptS && n > 0 && max_samples > ((int64_t)1 << 40) / n))
        return set_err(ctx, TD_ERR_ARG, "td_history_create: too large");
    td_history *h = new (std::nothrow) td_history();
    if (!h) return set_err(ctx, TD_ERR_NOMEM, "td_history_create: out of memory");
    h->ctx = ctx;
    h->max_samples = max_samples;
    h->max_cells = max_cells_total;
    h->n = n;
    const size_t S = (size_t)max_samples, C = (size_t)max_cells_total;
    const bool pts = with_ptS && n > 0;
    const size_t bytes = padded(4 * C * sizeof(double)) + padded((S + 1) * sizeof(long long)) +
                         padded(S * sizeof(long long)) + padded(S * sizeof(double)) + 3 * padded(S * sizeof(int)) +
                         (pts ? padded(S * (size_t)n * sizeof(double)) : 0);
    hipError_t e = hipSetDevice(ctx->device);
    servers_quiesce(nullptr);  // (the allocation and the memset below wait for the device)
    if (e == hipSuccess) e = hipMalloc(&h->block, bytes);
    if (e != hipSuccess) {
        delete h;
        return e == hipErrorOutOfMemory ? set_err(ctx, TD_ERR_NOMEM, "td_history_create: out of device memory")
                                        : hip_err(ctx, e, "td_history_create");
    }
    char *cur = static_cast<char *>(h->block);
    h->d.cells = carve<double>(cur, 4 * C);
    h->d.stride = (long long)max_cells_total;
    h->d.off = carve<long long>(cur, S + 1);
    h->d.iter = carve<long long>(cur, S);
    h->d.phi = carve<double>(cur, S);
    h->d.ncells = carve<int>(cur, S);
    h->d.action = carve<int>(cur, S);
    h->d.accept = carve<int>(cur, S);
    h->d.ptS = pts ? carve<double>(cur, S * (size_t)n) : nullptr;
    h->off.assign(1, 0);
    e = hipMemset(h->d.off, 0, sizeof(long long));
    if (e != hipSuccess) {
        (void)hipFree(h->block);
        delete h;
        return hip_err(ctx, e, "td_history_create: hipMemset");
    }
    *out = h;
    return TD_OK;
}

int td_history_destroy(td_history *h) {
    if (!h) return TD_OK;
    if (h->ctx && h->ctx->stream) (void)hipStreamSynchronize(h->ctx->stream);
    if (h->block) (void)hipFree(h->block);
    delete h;
    return TD_OK;
}

int td_history_clear(td_history *h) {
    if (!h) return TD_ERR_ARG;
    h->samples = 0;
    h->off.assign(1, 0);  // (off[0] on the device is 0 and never rewritten)
    return TD_OK;
}

int td_history_count(const td_history *h, int64_t *samples, int64_t *cells_used) {
    if (!h) return TD_ERR_ARG;
    if (samples) *samples = h->samples;
    if (cells_used) *cells_used = h->off[(size_t)h->samples];
    return TD_OK;
}

int td_history_read(td_history *h, int64_t first, int64_t count, int64_t *off_out, double *x, double *y, double *z,
                    double *zeta, int64_t cell_cap, double *phi, int64_t *iter, int32_t *action, int32_t *accept,
                    double *ptS_out) {
    if (!h) return TD_ERR_ARG;
    td_ctx *c = h->ctx;
    if (first < 0 || count < 0 || first > h->samples || count > h->samples - first)
        return set_err(c, TD_ERR_ARG, "td_history_read: samples out of range");
    if (ptS_out && !h->d.ptS && h->n > 0) return set_err(c, TD_ERR_ARG, "td_history_read: the history keeps no ptS");
    const int64_t a = h->off[(size_t)first], ncell = h->off[(size_t)(first + count)] - a;
    if (off_out)
        for (int64_t k = 0; k <= count; ++k) off_out[k] = h->off[(size_t)(first + k)] - a;
    if ((x || y || z || zeta) && cell_cap < ncell)
        return set_err(c, TD_ERR_ARG, "td_history_read: cell_cap smaller than the samples' cells");
    if (count == 0) return TD_OK;
    TD_HIP(c, hipSetDevice(c->device));
    servers_quiesce(nullptr);
    double *dst[4] = {x, y, z, zeta};
    for (int comp = 0; comp < 4; ++comp)
        if (dst[comp] && ncell > 0)
            TD_HIP(c, hipMemcpy(dst[comp], h->d.cells + comp * h->d.stride + a, sizeof(double) * (size_t)ncell,
                                hipMemcpyDeviceToHost));
    const size_t cnt = (size_t)count;
    if (phi) TD_HIP(c, hipMemcpy(phi, h->d.phi + first, sizeof(double) * cnt, hipMemcpyDeviceToHost));
    if (iter) TD_HIP(c, hipMemcpy(iter, h->d.iter + first, sizeof(int64_t) * cnt, hipMemcpyDeviceToHost));
    if (action) TD_HIP(c, hipMemcpy(action, h->d.action + first, sizeof(int32_t) * cnt, hipMemcpyDeviceToHost));
    if (accept) TD_HIP(c, hipMemcpy(accept, h->d.accept + first, sizeof(int32_t) * cnt, hipMemcpyDeviceToHost));
    if (ptS_out && h->d.ptS)
        TD_HIP(c, hipMemcpy(ptS_out, h->d.ptS + first * h->n, sizeof(double) * cnt * (size_t)h->n,
                            hipMemcpyDeviceToHost));
    return TD_OK;
}

int tdt_history_pack_chunk(void) { return kPackChunk; }

int tdt_history_pack(int device, double *cells, int64_t stride, int64_t slot0, int64_t slot_cells,
                     const int32_t *ncells, int64_t count, int64_t *off_out) {
    // (every check before any HIP call: the kernel tests no bound)
    if (!cells || !ncells || !off_out || stride < 1 || slot0 < 0 || slot_cells < 0 || count < 0 ||
        stride > ((int64_t)1 << 32) || count > ((int64_t)1 << 32))
        return set_err(nullptr, TD_ERR_ARG, "tdt_history_pack: bad arguments");
    if (count > 0 && slot_cells > (stride - slot0) / count)
        return set_err(nullptr, TD_ERR_ARG, "tdt_history_pack: the slots do not fit the stride");
    for (int64_t i = 0; i < count; ++i)
        if (ncells[i] < 0 || ncells[i] > slot_cells)
            return set_err(nullptr, TD_ERR_ARG, "tdt_history_pack: a sample larger than its slot");
    off_out[0] = slot0;
    if (count == 0) return TD_OK;
    if (device >= 0) TD_HIP(nullptr, hipSetDevice(device));
    servers_quiesce(nullptr);
    const size_t cb = sizeof(double) * 4 * (size_t)stride, nb = sizeof(int) * (size_t)count,
                 ob = sizeof(long long) * (size_t)(count + 1);
    double *d_cells = nullptr;
    int *d_n = nullptr;
    long long *d_off = nullptr;
    std::vector<long long> off((size_t)count + 1, 0);
    off[0] = slot0;
    hipError_t e = hipMalloc(&d_cells, cb);
    if (e == hipSuccess) e = hipMalloc(&d_n, nb);
    if (e == hipSuccess) e = hipMalloc(&d_off, ob);
    if (e == hipSuccess) e = hipMemcpy(d_cells, cells, cb, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_n, ncells, nb, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_off, off.data(), ob, hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = launch_history_pack(d_cells, (long long)stride, (long long)slot0, (long long)slot_cells, d_n,
                                (long long)count, d_off, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(cells, d_cells, cb, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(off.data(), d_off, ob, hipMemcpyDeviceToHost);
    if (d_cells) (void)hipFree(d_cells);
    if (d_n) (void)hipFree(d_n);
    if (d_off) (void)hipFree(d_off);
    if (e != hipSuccess) return hip_err(nullptr, e, "tdt_history_pack");
    for (int64_t i = 0; i <= count; ++i) off_out[i] = off[(size_t)i];
    return TD_OK;
}

}  // extern "C"
