// The device weight packer and the arena cache.
//
// Packer (me_ctx_set_weight_packer(ctx, 1)): me_load_weight copies a tensor's raw bytes, in the checkpoint's own layout and
// dtype, into a pinned staging buffer, queues the upload and ONE pack kernel on the context's stream and returns; a ring
// of kRing buffers, each guarded by an event, lets the host copy tensor i + 1 while tensor i crosses the link and is
// packed.  A device-pointer source is packed where it lies.  The index maps and conversions are weight_pack.h's, shared
// with the host packer, and the arena comes out byte for byte the host packer's.  Kernels, all destination-major:
//   pack_flat16_kernel   K_MAT_16 ([W | W] per row when dup): eight destination elements per thread, one 16-byte store
//   pack_conv16_kernel   K_CONV_16: per output channel and tile of 64 input channels the contiguous [ci][kk] run is read
//                        coalesced, turned in LDS and written as kk (x dup) rows of 64 contiguous elements (16-byte stores
//                        when Cin is a multiple of 8, as every slot of the model is; 2-byte lanes of one run otherwise)
//   pack_convt16_kernel  K_CONVT_16: a 64 ci x 16 co tile; per ci the contiguous [co][q] run of 64 elements is read
//                        coalesced, transposed through LDS (rows padded to 33 words: the column-wise writes of the load
//                        side and the row-wise reads of the store side both spread over the banks) and written as 4 x 16
//                        (x dup) rows of 64 contiguous elements
//   pack_flat32_kernel   K_VEC_F32, K_CONVK_F32
// An f16 source into an f16 arena's plain matrix slot, and an f32 source into an f32 slot, need no kernel: the upload lands
// in the slot.
//
// Cache (me_save_weight_arena / me_load_weight_arena / me_load_checkpoint_cached): a 256-byte header (weight_pack.h) and
// the raw arena.  The payload's checksum is a sum of mixed (position, word) terms modulo 2^64, computed on the device by
// block sums and integer atomic adds -- the same value in any order.
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <cstdio>
#include <cstring>
#include <thread>

#include "../../include/matrix_eyes_hip_ops.h"
#include "weight_pack_state.h"

using namespace me;
using namespace me_pack;

namespace {

constexpr int kThreads = kTileThreads;

template <int SRC, int DST>
__global__ __launch_bounds__(kThreads) void pack_flat16_kernel(Shape s, const void* __restrict__ src, uint16_t* __restrict__ dst,
                                                               int vec) {
    const int64_t base = ((int64_t)blockIdx.x * kThreads + threadIdx.x) * 8;
    if (base >= s.dst_elems) return;
    if (vec && base + 8 <= s.dst_elems) {
        uint32_t w[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t lo = src_get16(src, SRC, src_index(s, base + 2 * j), DST);
            const uint32_t hi = src_get16(src, SRC, src_index(s, base + 2 * j + 1), DST);
            w[j] = lo | (hi << 16);
        }
        *reinterpret_cast<uint4*>(dst + base) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
        const int64_t end = base + 8 < s.dst_elems ? base + 8 : s.dst_elems;
        for (int64_t d = base; d < end; ++d) dst[d] = src_get16(src, SRC, src_index(s, d), DST);
    }
}

template <int SRC>
__global__ __launch_bounds__(kThreads) void pack_flat32_kernel(Shape s, const void* __restrict__ src, uint32_t* __restrict__ dst) {
    const int64_t d = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (d < s.dst_elems) dst[d] = src_get32(src, SRC, src_index(s, d));
}

// eight 16-bit elements of the LDS tile (4-byte aligned: the pitch and the channel offset are even) as one 16-byte store
__device__ inline void store8(uint16_t* dst, const uint16_t* lds) {
    const uint32_t* w = reinterpret_cast<const uint32_t*>(lds);
    *reinterpret_cast<uint4*>(dst) = make_uint4(w[0], w[1], w[2], w[3]);
}

// grid (ceil(Cin / kTileCi), Cout); the work items are weight_pack.h's
template <int SRC, int DST>
__global__ __launch_bounds__(kThreads) void pack_conv16_kernel(Shape s, const void* __restrict__ src, uint16_t* __restrict__ dst, int vec) {
    __shared__ __align__(16) uint16_t tile[kConvTileElems];
    const int64_t bx = blockIdx.x, by = blockIdx.y;
    for (int i = (int)threadIdx.x, n = conv_tile_loads(s, bx); i < n; i += kThreads) {
        const TileRef r = conv_tile_load(s, bx, by, i);
        tile[r.lds] = src_get16(src, SRC, r.g, DST);
    }
    __syncthreads();
    if (vec) {  // Cin a multiple of 8 and dst 16-byte aligned: eight input channels per lane, one 16-byte store
        for (int i = (int)threadIdx.x, n = conv_tile_stores(s) / 8; i < n; i += kThreads) {
            TileRef r;
            if (conv_tile_store(s, bx, by, tile_store8_item(i), &r)) store8(dst + r.g, tile + r.lds);
        }
        return;
    }
    for (int i = (int)threadIdx.x, n = conv_tile_stores(s); i < n; i += kThreads) {
        TileRef r;
        if (conv_tile_store(s, bx, by, i, &r)) dst[r.g] = tile[r.lds];
    }
}

// grid (ceil(Cin / kTileCi), ceil(Cout / kTileCo))
template <int SRC, int DST>
__global__ __launch_bounds__(kThreads) void pack_convt16_kernel(Shape s, const void* __restrict__ src, uint16_t* __restrict__ dst, int vec) {
    __shared__ __align__(16) uint16_t tile[kConvtTileElems];
    const int64_t bx = blockIdx.x, by = blockIdx.y;
    for (int i = (int)threadIdx.x, n = convt_tile_loads(s, bx, by); i < n; i += kThreads) {
        const TileRef r = convt_tile_load(s, bx, by, i);
        tile[r.lds] = src_get16(src, SRC, r.g, DST);
    }
    __syncthreads();
    if (vec) {
        for (int i = (int)threadIdx.x, n = convt_tile_stores(s, by) / 8; i < n; i += kThreads) {
            TileRef r;
            if (convt_tile_store(s, bx, by, tile_store8_item(i), &r)) store8(dst + r.g, tile + r.lds);
        }
        return;
    }
    for (int i = (int)threadIdx.x, n = convt_tile_stores(s, by); i < n; i += kThreads) {
        TileRef r;
        if (convt_tile_store(s, bx, by, i, &r)) dst[r.g] = tile[r.lds];
    }
}

__global__ __launch_bounds__(kThreads) void arena_checksum_kernel(const uint32_t* __restrict__ words, uint64_t nwords,
                                                                  unsigned long long* out) {
    __shared__ unsigned long long part[kThreads];
    unsigned long long sum = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < nwords; i += (uint64_t)gridDim.x * kThreads)
        sum += checksum_term(i, words[i]);
    part[threadIdx.x] = sum;
    __syncthreads();
    for (int step = kThreads / 2; step > 0; step >>= 1) {
        if ((int)threadIdx.x < step) part[threadIdx.x] += part[threadIdx.x + step];
        __syncthreads();
    }
    if (threadIdx.x == 0) atomicAdd(out, part[0]);
}

template <int SRC, int DST>
void launch16(const Shape& s, const void* src, void* dst, hipStream_t stream) {
    uint16_t* d = (uint16_t*)dst;
    const int vec = ((uintptr_t)dst & 15) == 0 ? 1 : 0;
    const int vec_rows = vec && tile_store8_ok(s) ? 1 : 0;   // every destination row starts on a 16-byte boundary
    if (s.kind == K_CONV_16 && s.Cout <= 65535) {
        hipLaunchKernelGGL((pack_conv16_kernel<SRC, DST>), dim3((unsigned)cdiv(s.Cin, kTileCi), (unsigned)s.Cout), dim3(kThreads), 0,
                           stream, s, src, d, vec_rows);
    } else if (s.kind == K_CONVT_16 && cdiv(s.Cout, kTileCo) <= 65535) {
        hipLaunchKernelGGL((pack_convt16_kernel<SRC, DST>), dim3((unsigned)cdiv(s.Cin, kTileCi), (unsigned)cdiv(s.Cout, kTileCo)),
                           dim3(kThreads), 0, stream, s, src, d, vec_rows);
    } else {
        hipLaunchKernelGGL((pack_flat16_kernel<SRC, DST>), dim3((unsigned)cdiv(cdiv(s.dst_elems, 8), kThreads)), dim3(kThreads), 0,
                           stream, s, src, d, vec);
    }
}

template <int SRC>
void launch_src(const Shape& s, int32_t dst_dtype, const void* src, void* dst, hipStream_t stream) {
    if (s.kind == K_VEC_F32 || s.kind == K_CONVK_F32)
        hipLaunchKernelGGL((pack_flat32_kernel<SRC>), dim3((unsigned)cdiv(s.dst_elems, kThreads)), dim3(kThreads), 0, stream, s, src,
                           (uint32_t*)dst);
    else if (dst_dtype == D_BF16)
        launch16<SRC, D_BF16>(s, src, dst, stream);
    else
        launch16<SRC, D_F16>(s, src, dst, stream);
}

int pack_threads() {
    static const int n = std::max(1, std::min(16, env_int("ME_PACK_THREADS", 4)));
    return n;
}

// fn(offset, length) over [0, bytes) in pieces, by up to pack_threads() host threads (one per 4 MiB at least)
template <class F>
void parallel_bytes(size_t bytes, F fn) {
    const int n = (int)std::min<size_t>((size_t)pack_threads(), std::max<size_t>(1, bytes >> 22));
    if (n <= 1) return fn((size_t)0, bytes);
    const size_t piece = ((bytes + n - 1) / n + 4095) & ~(size_t)4095;
    std::vector<std::thread> pool;
    for (int t = 1; t < n; ++t) {
        const size_t lo = std::min(bytes, piece * t), hi = std::min(bytes, lo + piece);
        if (hi > lo) pool.emplace_back([=]() { fn(lo, hi - lo); });
    }
    fn((size_t)0, std::min(bytes, piece));
    for (std::thread& th : pool) th.join();
}

hipEvent_t take_event(WeightPackState& st) {
    if (st.events_used == st.event_pool.size()) {
        hipEvent_t e = nullptr;
        ME_HIP(hipEventCreate(&e));
        st.event_pool.push_back(e);
    }
    return st.event_pool[st.events_used++];
}

hipEvent_t mark(WeightPackState& st, hipStream_t stream) {
    hipEvent_t e = take_event(st);
    ME_HIP(hipEventRecord(e, stream));
    return e;
}

// the next ring buffer with room for `need` bytes (grown to `cap`), free of the launch that last read it
WeightPackState::Buf& acquire(me_ctx* ctx, WeightPackState& st, size_t need, size_t cap) {
    WeightPackState::Buf& b = st.ring[st.next];
    st.next = (st.next + 1) % WeightPackState::kRing;
    if (b.busy) {
        ME_HIP(hipEventSynchronize(b.done));
        b.busy = false;
    }
    if (b.bytes < need) {
        if (b.pinned) ME_HIP(hipHostFree(b.pinned));
        if (b.dev) ME_HIP(hipFree(b.dev));
        b.pinned = b.dev = nullptr, b.bytes = 0;
        const size_t bytes = (std::max(need, cap) + 4095) & ~(size_t)4095;
        ME_HIP(hipHostMalloc((void**)&b.pinned, bytes, hipHostMallocDefault));
        ME_HIP(hipMalloc((void**)&b.dev, bytes));
        b.bytes = bytes;
    }
    if (!b.done) ME_HIP(hipEventCreateWithFlags(&b.done, hipEventDisableTiming));
    (void)ctx;
    return b;
}

void release(me_ctx* ctx, WeightPackState& st, WeightPackState::Buf& b) {
    ME_HIP(hipEventRecord(b.done, ctx->stream));
    b.busy = true;
    st.pending = true;
}

Shape slot_shape(const WeightSlot& s) {
    Shape sh;
    const char* why = make_shape((int32_t)s.kind, s.dup ? 1 : 0, s.dims.data(), (int32_t)s.dims.size(), &sh);
    ME_CHECK(!why, ME_ERR_BAD_SHAPE, "internal: slot %s: %s", s.name.c_str(), why);
    ME_CHECK((size_t)sh.dst_bytes == s.bytes, ME_ERR_BAD_SHAPE, "internal: slot %s holds %zu bytes, its packing %lld", s.name.c_str(),
             s.bytes, (long long)sh.dst_bytes);
    return sh;
}

void mark_unloaded(me_ctx* ctx) {
    for (WeightSlot& s : ctx->slots) s.loaded = false;
    ctx->finalized = false;
    ctx->factor_keep.clear();
    ctx->drop_graph(), ++ctx->weights_generation;
}

const char* dtype_name(const me_ctx* ctx) { return ctx->fp8 ? "fp8" : (ctx->dtype == ME_DTYPE_BF16 ? "bf16" : "f16"); }

ArenaExpect expect_of(const me_ctx* ctx) {
    static_assert(sizeof(me_model_config) == 4 * kArenaConfigWords, "me_model_config changed: bump ME_ARENA_FORMAT and kArenaConfigWords");
    ArenaExpect e;
    e.dtype = ctx->fp8 ? ME_DTYPE_FP8 : ctx->dtype;
    e.split_mask = ctx->split_mask;
    memcpy(e.config, &ctx->cfg, sizeof e.config);
    e.layout = ctx->arena_layout_hash();
    e.arena_bytes = ctx->arena_bytes;
    return e;
}

struct Stamp {
    bool exists = false;
    int64_t size = -1, mtime_ns = -1;
};
Stamp stamp_of(const char* path) {
    Stamp s;
    struct stat st;
    if (path && stat(path, &st) == 0) {
        s.exists = true;
        s.size = (int64_t)st.st_size;
        s.mtime_ns = (int64_t)st.st_mtim.tv_sec * 1000000000ll + (int64_t)st.st_mtim.tv_nsec;
    }
    return s;
}

// the checksum of the arena as it is on the device, behind everything queued on the stream (synchronises)
uint64_t arena_checksum(me_ctx* ctx, WeightPackState& st, double* kernel_ms) {
    if (!st.checksum_dev) ME_HIP(hipMalloc((void**)&st.checksum_dev, 256));
    if (!st.checksum_host) ME_HIP(hipHostMalloc((void**)&st.checksum_host, 64, hipHostMallocDefault));
    ME_HIP(hipMemsetAsync(st.checksum_dev, 0, 8, ctx->stream));
    hipEvent_t e0 = mark(st, ctx->stream);
    const uint64_t nwords = ctx->arena_bytes / 4;
    const unsigned grid = (unsigned)std::min<uint64_t>(2048, std::max<uint64_t>(1, cdiv((int64_t)nwords, kThreads)));
    hipLaunchKernelGGL(arena_checksum_kernel, dim3(grid), dim3(kThreads), 0, ctx->stream, (const uint32_t*)ctx->arena, nwords,
                       (unsigned long long*)st.checksum_dev);
    ME_HIP(hipGetLastError());
    hipEvent_t e1 = mark(st, ctx->stream);
    ME_HIP(hipMemcpyAsync(st.checksum_host, st.checksum_dev, 8, hipMemcpyDeviceToHost, ctx->stream));
    ME_HIP(hipStreamSynchronize(ctx->stream));
    if (kernel_ms) {
        float ms = 0.f;
        ME_HIP(hipEventElapsedTime(&ms, e0, e1));
        *kernel_ms += ms;
    }
    return *st.checksum_host;
}

// The verdict on the cache file at `path` for this context; `source` the checkpoint's stamp.  file_bytes 0: no such file.
ArenaVerdict read_verdict(me_ctx* ctx, const char* path, const Stamp& source, uint64_t* file_bytes) {
    *file_bytes = 0;
    FILE* f = fopen(path, "rb");
    ME_CHECK(f, ME_ERR_IO, "cannot open %s: %s", path, strerror(errno));
    char head[kArenaHeaderBytes];
    const size_t have = fread(head, 1, sizeof head, f);
    fclose(f);
    const Stamp self = stamp_of(path);
    *file_bytes = (uint64_t)std::max<int64_t>(0, self.size);
    return arena_header_check(head, have, *file_bytes, expect_of(ctx), source.exists, source.size, source.mtime_ns, nullptr);
}

[[noreturn]] void fail_damaged(me_ctx* ctx, const char* path, const char* why) {
    mark_unloaded(ctx);
    fail(ME_ERR_IO, "%s: damaged weight arena cache (%s); delete the file and the checkpoint will be packed again", path, why);
}

// header valid: the payload into the arena through the pinned ring, checked on the device, then adopted
void load_arena_payload(me_ctx* ctx, const char* path, uint64_t file_bytes) {
    WeightPackState& st = weight_pack_state(ctx);
    weight_pack_sync(ctx);
    st.cur = WeightLoadReport();
    st.open = false;
    WeightLoadReport rep;
    rep.where = WS_CACHE;
    rep.tensors = (int64_t)ctx->slots.size();
    mark_unloaded(ctx);   // from here on the arena is neither the old weights nor yet the new ones
    FILE* f = fopen(path, "rb");
    ME_CHECK(f, ME_ERR_IO, "cannot open %s: %s", path, strerror(errno));
    const int fd = fileno(f);
    ArenaHeader h;
    const bool got_head = pread(fd, &h, sizeof h, 0) == (ssize_t)sizeof h;
    constexpr size_t kChunk = (size_t)32 << 20;
    std::atomic<int> failed{0};
    std::vector<std::pair<hipEvent_t, hipEvent_t>> uploads;
    try {
        ME_CHECK(got_head, ME_ERR_IO, "%s: cannot read the header", path);
        for (size_t off = 0; off < ctx->arena_bytes && !failed; off += kChunk) {
            const size_t n = std::min(kChunk, ctx->arena_bytes - off);
            WeightPackState::Buf& b = acquire(ctx, st, n, kChunk);
            const double t0 = wall_ms();
            parallel_bytes(n, [&](size_t lo, size_t len) {
                size_t done = 0;
                while (done < len) {
                    const ssize_t r = pread(fd, b.pinned + lo + done, len - done, (off_t)(kArenaHeaderBytes + off + lo + done));
                    if (r <= 0) {
                        failed = 1;
                        return;
                    }
                    done += (size_t)r;
                }
            });
            rep.ms[0] += wall_ms() - t0;
            if (failed) break;
            hipEvent_t e0 = mark(st, ctx->stream);
            ME_HIP(hipMemcpyAsync(ctx->arena + off, b.pinned, n, hipMemcpyHostToDevice, ctx->stream));
            uploads.emplace_back(e0, mark(st, ctx->stream));
            release(ctx, st, b);
        }
    } catch (...) {
        fclose(f);
        throw;
    }
    fclose(f);
    if (failed) {
        weight_pack_sync(ctx);
        fail_damaged(ctx, path, "the file could not be read to its end");
    }
    const uint64_t sum = arena_checksum(ctx, st, &rep.ms[2]);
    for (auto& u : uploads) {
        float ms = 0.f;
        ME_HIP(hipEventElapsedTime(&ms, u.first, u.second));
        rep.ms[1] += ms;
    }
    weight_pack_sync(ctx);
    if (sum != h.checksum) fail_damaged(ctx, path, "checksum mismatch");
    rep.bytes_read = (int64_t)file_bytes;
    rep.bytes_uploaded = (int64_t)ctx->arena_bytes;
    const double t0 = wall_ms();
    adopt_weights(ctx);
    rep.ms[3] = wall_ms() - t0;
    st.last = rep, st.reported = true;
}

}  // namespace

namespace me {

WeightPackState& weight_pack_state(me_ctx* ctx) {
    if (!ctx->wp) ctx->wp = new WeightPackState();
    return *ctx->wp;
}

WeightLoadReport& weight_load_begin(me_ctx* ctx) {
    WeightPackState& st = weight_pack_state(ctx);
    if (!st.open) st.cur = WeightLoadReport(), st.open = true;
    return st.cur;
}

void free_weight_pack(me_ctx* ctx) {
    WeightPackState* st = ctx->wp;
    if (!st) return;
    for (WeightPackState::Buf& b : st->ring) {
        if (b.pinned) (void)hipHostFree(b.pinned);
        if (b.dev) (void)hipFree(b.dev);
        if (b.done) (void)hipEventDestroy(b.done);
    }
    for (hipEvent_t e : st->event_pool) (void)hipEventDestroy(e);
    if (st->checksum_dev) (void)hipFree(st->checksum_dev);
    if (st->checksum_host) (void)hipHostFree(st->checksum_host);
    delete st;
    ctx->wp = nullptr;
}

void weight_pack_launch(const Shape& s, int32_t dst_dtype, const void* src_dev, int32_t src_dtype, void* dst_dev, hipStream_t stream) {
    switch (src_dtype) {
        case W_F32: launch_src<W_F32>(s, dst_dtype, src_dev, dst_dev, stream); break;
        case W_F16: launch_src<W_F16>(s, dst_dtype, src_dev, dst_dev, stream); break;
        case W_BF16: launch_src<W_BF16>(s, dst_dtype, src_dev, dst_dev, stream); break;
        default: launch_src<W_F64>(s, dst_dtype, src_dev, dst_dev, stream); break;
    }
    ME_HIP(hipGetLastError());
}

void weight_pack_sync(me_ctx* ctx) {
    WeightPackState* st = ctx->wp;
    if (!st) return;
    if (st->pending || !st->marks.empty()) ME_HIP(hipStreamSynchronize(ctx->stream));
    for (const WeightPackState::Marks& m : st->marks) {
        float ms = 0.f;
        if (m.e[0] && m.e[1]) {
            ME_HIP(hipEventElapsedTime(&ms, m.e[0], m.e[1]));
            st->cur.ms[1] += ms;
        }
        if (m.e[1] && m.e[2]) {
            ME_HIP(hipEventElapsedTime(&ms, m.e[1], m.e[2]));
            st->cur.ms[2] += ms;
        }
    }
    st->marks.clear();
    st->events_used = 0;
    for (WeightPackState::Buf& b : st->ring) b.busy = false;
    st->pending = false;
}

void device_pack_weight(me_ctx* ctx, WeightSlot& s, const void* data, int32_t weight_dtype) {
    WeightPackState& st = weight_pack_state(ctx);
    const Shape sh = slot_shape(s);
    const size_t src_bytes = (size_t)sh.numel * src_elem_size(weight_dtype);
    char* dst = ctx->arena + s.offset;
    // the source's bytes are the slot's bytes: no kernel
    const bool direct = (s.kind == PK_MAT_16 && !s.dup && weight_dtype == ME_WEIGHT_F16 && ctx->dtype == ME_DTYPE_F16) ||
                        (s.kind == PK_VEC_F32 && weight_dtype == ME_WEIGHT_F32);
    WeightLoadReport& rep = st.cur;
    WeightPackState::Marks m;
    if (is_device_ptr(data)) {
        m.e[1] = mark(st, ctx->stream);
        if (direct)
            ME_HIP(hipMemcpyAsync(dst, data, src_bytes, hipMemcpyDeviceToDevice, ctx->stream));
        else
            weight_pack_launch(sh, ctx->dtype, data, weight_dtype, dst, ctx->stream);
        m.e[2] = mark(st, ctx->stream);
        st.pending = true;
    } else {
        size_t cap = 0;   // the largest tensor of the model in this source type: the ring is sized once
        for (const WeightSlot& o : ctx->slots) cap = std::max(cap, (size_t)o.numel() * src_elem_size(weight_dtype));
        WeightPackState::Buf& b = acquire(ctx, st, src_bytes, cap);
        const double t0 = wall_ms();
        const char* from = (const char*)data;
        parallel_bytes(src_bytes, [&](size_t lo, size_t len) { memcpy(b.pinned + lo, from + lo, len); });
        rep.ms[0] += wall_ms() - t0;
        m.e[0] = mark(st, ctx->stream);
        ME_HIP(hipMemcpyAsync(direct ? dst : b.dev, b.pinned, src_bytes, hipMemcpyHostToDevice, ctx->stream));
        m.e[1] = mark(st, ctx->stream);
        if (!direct) {
            weight_pack_launch(sh, ctx->dtype, b.dev, weight_dtype, dst, ctx->stream);
            m.e[2] = mark(st, ctx->stream);
        }
        release(ctx, st, b);
        rep.bytes_uploaded += (int64_t)src_bytes;
    }
    st.marks.push_back(m);
}

std::string weight_cache_path(me_ctx* ctx, const char* checkpoint_path) {
    std::string out(strlen(checkpoint_path) + 64, '\0');
    const int64_t n = arena_cache_path(checkpoint_path, dtype_name(ctx), ctx->arena_layout_hash(), &out[0], out.size());
    ME_CHECK(n >= 0, ME_ERR_BAD_ARG, "internal: cache path");
    out.resize((size_t)n);
    return out;
}

void save_weight_arena(me_ctx* ctx, const char* path, const char* source_path) {
    ME_CHECK(path, ME_ERR_BAD_ARG, "me_save_weight_arena: null path");
    ME_CHECK(ctx->finalized, ME_ERR_NOT_READY, "me_save_weight_arena: the weights are not finalized");
    WeightPackState& st = weight_pack_state(ctx);
    weight_pack_sync(ctx);
    const double t0 = wall_ms();
    const uint64_t sum = arena_checksum(ctx, st, nullptr);
    st.events_used = 0;
    const Stamp src = stamp_of(source_path);
    const size_t total = kArenaHeaderBytes + ctx->arena_bytes;
    char* host = nullptr;
    ME_HIP(hipHostMalloc((void**)&host, total, hipHostMallocDefault));
    const std::string tmp = std::string(path) + ".tmp." + std::to_string((long long)getpid());
    try {
        arena_header_write(expect_of(ctx), src.size, src.mtime_ns, sum, host);
        ME_HIP(hipMemcpyAsync(host + kArenaHeaderBytes, ctx->arena, ctx->arena_bytes, hipMemcpyDeviceToHost, ctx->stream));
        ME_HIP(hipStreamSynchronize(ctx->stream));
        write_bytes_parallel(tmp, host, total);
        ME_CHECK(rename(tmp.c_str(), path) == 0, ME_ERR_IO, "cannot rename %s to %s: %s", tmp.c_str(), path, strerror(errno));
    } catch (...) {
        (void)hipHostFree(host);
        (void)unlink(tmp.c_str());
        throw;
    }
    ME_HIP(hipHostFree(host));
    if (st.reported) st.last.ms[4] = wall_ms() - t0;
}

void load_weight_arena(me_ctx* ctx, const char* path, const char* source_path) {
    ME_CHECK(path, ME_ERR_BAD_ARG, "me_load_weight_arena: null path");
    uint64_t file_bytes = 0;
    const ArenaVerdict v = read_verdict(ctx, path, stamp_of(source_path), &file_bytes);
    if (v == ARENA_STALE_FORMAT || v == ARENA_STALE_SOURCE)
        fail(ME_ERR_IO, "%s: stale weight arena cache (%s)", path, arena_verdict_text(v));
    if (v != ARENA_OK) fail_damaged(ctx, path, arena_verdict_text(v));
    load_arena_payload(ctx, path, file_bytes);
}

void load_checkpoint_cached(me_ctx* ctx, const char* checkpoint_path, bool convert, int32_t* where) {
    ME_CHECK(checkpoint_path, ME_ERR_BAD_ARG, "me_load_checkpoint_cached: null path");
    const std::string cache = weight_cache_path(ctx, checkpoint_path);
    if (stamp_of(cache.c_str()).exists) {
        uint64_t file_bytes = 0;
        const ArenaVerdict v = read_verdict(ctx, cache.c_str(), stamp_of(checkpoint_path), &file_bytes);
        if (v == ARENA_OK) {
            load_arena_payload(ctx, cache.c_str(), file_bytes);   // the checkpoint is not opened
            if (where) *where = (int32_t)WS_CACHE;
            return;
        }
        if (v != ARENA_STALE_FORMAT && v != ARENA_STALE_SOURCE) fail_damaged(ctx, cache.c_str(), arena_verdict_text(v));
        // a deliberate deviation: the reference would load the stale file (mod.rs:225-227)
        fprintf(stderr, "matrix-eyes-hip: %s: stale weight arena cache (%s): loading %s%s\n", cache.c_str(), arena_verdict_text(v),
                checkpoint_path, convert ? " and rewriting the cache" : "");
    }
    load_checkpoint_pt(ctx, checkpoint_path);
    if (where) *where = ctx->weight_packer == 1 ? (int32_t)WS_PT_DEVICE : (int32_t)WS_PT_HOST;
    if (convert) save_weight_arena(ctx, cache.c_str(), checkpoint_path);
}

}  // namespace me

extern "C" {

int32_t me_ctx_set_weight_packer(me_ctx* ctx, int32_t packer) {
    ME_API_BEGIN(ctx)
    ME_CHECK(packer == 0 || packer == 1, ME_ERR_BAD_ARG, "me_ctx_set_weight_packer: packer %d (0 host, 1 device)", packer);
    weight_pack_sync(ctx);
    ctx->weight_packer = packer;
    ME_API_END(ctx)
}

int32_t me_save_weight_arena(me_ctx* ctx, const char* path, const char* source_path) {
    ME_API_BEGIN(ctx)
    save_weight_arena(ctx, path, source_path);
    ME_API_END(ctx)
}

int32_t me_load_weight_arena(me_ctx* ctx, const char* path, const char* source_path) {
    ME_API_BEGIN(ctx)
    load_weight_arena(ctx, path, source_path);
    ME_API_END(ctx)
}

int64_t me_weight_cache_path(const me_ctx* ctx, const char* checkpoint_path, char* buf, int64_t cap) {
    if (!ctx || !checkpoint_path || !buf || cap <= 0) return -1;
    return arena_cache_path(checkpoint_path, dtype_name(ctx), ctx->arena_layout_hash(), buf, (size_t)cap);
}

int32_t me_load_checkpoint_cached(me_ctx* ctx, const char* checkpoint_path, int32_t convert, int32_t* where) {
    ME_API_BEGIN(ctx)
    load_checkpoint_cached(ctx, checkpoint_path, convert != 0, where);
    ME_API_END(ctx)
}

int32_t me_last_weight_load(me_ctx* ctx, int64_t info[4], double ms[5]) {
    ME_API_BEGIN(ctx)
    ME_CHECK(info && ms, ME_ERR_BAD_ARG, "me_last_weight_load: null pointer");
    ME_CHECK(ctx->wp && ctx->wp->reported, ME_ERR_NOT_READY, "me_last_weight_load: no weights have been loaded and finalized");
    const WeightLoadReport& r = ctx->wp->last;
    info[0] = r.where, info[1] = r.tensors, info[2] = r.bytes_read, info[3] = r.bytes_uploaded;
    for (int i = 0; i < 5; ++i) ms[i] = r.ms[i];
    ME_API_END(ctx)
}

int32_t me_op_weight_pack(me_ctx* ctx, int32_t kind, int32_t dup, const int64_t* dims, int32_t ndim, const void* src,
                          int32_t src_dtype, void* dst) {
    ME_API_BEGIN(ctx)
    ME_CHECK(src && dst && dims, ME_ERR_BAD_ARG, "me_op_weight_pack: null pointer");
    ME_CHECK(src_dtype >= ME_WEIGHT_F32 && src_dtype <= ME_WEIGHT_F64, ME_ERR_BAD_ARG, "me_op_weight_pack: source dtype %d", src_dtype);
    Shape s;
    const char* why = make_shape(kind, dup, dims, ndim, &s);
    ME_CHECK(!why, ME_ERR_BAD_SHAPE, "me_op_weight_pack: kind %d: %s", kind, why);
    const void* sdev = to_device(ctx, src, (size_t)s.numel * src_elem_size(src_dtype), "op.wpack.src");
    OutBuf o = out_buf(ctx, dst, (size_t)s.dst_bytes, "op.wpack.dst");
    weight_pack_launch(s, ctx->dtype, sdev, src_dtype, o.dev, ctx->stream);
    finish(ctx, o);
    ME_API_END(ctx)
}

int32_t me_op_weight_pack_host(int32_t dtype, int32_t kind, int32_t dup, const int64_t* dims, int32_t ndim, const void* src,
                               int32_t src_dtype, void* dst) {
    if (!src || !dst || !dims) return -1;
    if ((dtype != ME_DTYPE_F16 && dtype != ME_DTYPE_BF16) || src_dtype < ME_WEIGHT_F32 || src_dtype > ME_WEIGHT_F64) return -2;
    Shape s;
    if (make_shape(kind, dup, dims, ndim, &s)) return -3;
    pack_host(s, dtype, src, src_dtype, dst);
    return 0;
}

}  // extern "C"
