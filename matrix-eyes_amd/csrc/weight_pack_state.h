// What a context keeps for its weight loads beyond the arena itself (me_ctx::wp): the device packer's staging ring, the
// timing marks of the load in progress and the report of the last one (me_last_weight_load).  Included by weights.hip,
// weight_pack.hip and api.hip only.
#pragma once
#include <chrono>

#include "model.h"
#include "weight_pack.h"

namespace me {

enum WeightSource : int64_t { WS_PT_HOST = 0, WS_PT_DEVICE = 1, WS_CACHE = 2 };

struct WeightLoadReport {
    int64_t where = WS_PT_HOST;
    int64_t tensors = 0, bytes_read = 0, bytes_uploaded = 0;
    // [0] read and stage (host wall clock: the host packer's loops, or the copies into the pinned ring), [1] upload,
    // [2] pack kernels (HIP events with the device packer and the cache), [3] compose and finalise, [4] cache write
    double ms[5] = {0, 0, 0, 0, 0};
};

struct WeightPackState {
    // Ring of staging buffers, each a pinned host buffer and its device twin, sized to the largest tensor of the model in
    // the source type at hand (f64: 34 MB at full size).  `done` is recorded behind the last launch that reads a buffer;
    // the next user of the buffer waits for it on the host.
    static constexpr int kRing = 3;
    struct Buf {
        char* pinned = nullptr;
        char* dev = nullptr;
        size_t bytes = 0;
        hipEvent_t done = nullptr;
        bool busy = false;
    };
    Buf ring[kRing];
    int next = 0;
    bool pending = false;   // launches queued since the last weight_pack_sync
    // timing marks of the load in progress: {before the upload, behind it, behind the kernel}; a null mark: no such leg
    struct Marks {
        hipEvent_t e[3] = {nullptr, nullptr, nullptr};
    };
    std::vector<Marks> marks;
    std::vector<hipEvent_t> event_pool;
    size_t events_used = 0;
    uint64_t* checksum_dev = nullptr;   // the word the checksum kernel adds into
    uint64_t* checksum_host = nullptr;  // pinned
    WeightLoadReport cur, last;
    bool open = false;       // `cur` is being filled (a load_weight since the last finalize)
    bool reported = false;   // `last` is valid
};

inline double wall_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// the context's state, created on first use; the report of a load that starts here
WeightPackState& weight_pack_state(me_ctx* ctx);
WeightLoadReport& weight_load_begin(me_ctx* ctx);

// one pack kernel on `stream`: device pointers, `dst` the slot (or any buffer of s.dst_bytes)
void weight_pack_launch(const me_pack::Shape& s, int32_t dst_dtype, const void* src_dev, int32_t src_dtype, void* dst_dev,
                        hipStream_t stream);

// the arena cache (weight_pack.hip)
void save_weight_arena(me_ctx* ctx, const char* path, const char* source_path);
void load_weight_arena(me_ctx* ctx, const char* path, const char* source_path);
std::string weight_cache_path(me_ctx* ctx, const char* checkpoint_path);
// where: WeightSource
void load_checkpoint_cached(me_ctx* ctx, const char* checkpoint_path, bool convert, int32_t* where);

}  // namespace me
