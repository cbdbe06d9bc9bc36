// Files written from host memory (declared in model.h): a file of sections serialised on the host, a finished buffer
// written whole, and the write-behind slots of me_ctx_set_write_behind.  Host code only; a .hip unit because the slots'
// staging buffers are pinned (hipHostMalloc).  The mesh writers (mesh_writer.hip) and the arena cache (weight_pack.hip)
// write through here.
#include <atomic>
#include <cerrno>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <unistd.h>
#include <vector>

#include "model.h"

namespace me {

namespace {

struct FileSink {
    FILE* f = nullptr;
    std::string buf;
    explicit FileSink(const std::string& path) {
        f = fopen(path.c_str(), "wb");
        ME_CHECK(f, ME_ERR_IO, "cannot create %s: %s", path.c_str(), strerror(errno));
        buf.reserve(1 << 20);
    }
    ~FileSink() {
        if (f) fclose(f);
    }
    void flush_if_full() {  // WRITE_BUFFER_SIZE, output.rs:383
        if (buf.size() >= (1u << 20)) flush();
    }
    void flush() {
        if (!buf.empty()) {
            ME_CHECK(fwrite(buf.data(), 1, buf.size(), f) == buf.size(), ME_ERR_IO, "write failed: %s",
                     strerror(errno));
            buf.clear();
        }
    }
    void close() {
        flush();
        const int r = fclose(f);
        f = nullptr;
        ME_CHECK(r == 0, ME_ERR_IO, "close failed: %s", strerror(errno));
    }
};

// work(c) for every c in [0, n), on up to `nthreads` threads, the caller's among them.  work returns 0 or an errno; a
// thread stops at its first failure, and one of the failures (0: none) is returned.
template <typename Work>
int for_each_chunk(int64_t n, int nthreads, Work work) {
    std::atomic<int64_t> next{0};
    std::atomic<int> failed{0};
    auto run = [&]() {
        for (int64_t c; (c = next.fetch_add(1)) < n;)
            if (const int e = work(c)) {
                failed = e;
                return;
            }
    };
    std::vector<std::thread> pool;
    for (int t = 1; t < nthreads; ++t) pool.emplace_back(run);
    run();
    for (std::thread& t : pool) t.join();
    return failed;
}

// all of `bytes` at offset `at`; 0 or the errno (a write of nothing is EIO)
int pwrite_all(int fd, const char* data, size_t bytes, off_t at) {
    for (size_t done = 0; done < bytes;) {
        const ssize_t r = pwrite(fd, data + done, bytes - done, at + (off_t)done);
        if (r <= 0) return r < 0 ? errno : EIO;
        done += (size_t)r;
    }
    return 0;
}

// One section of the file (all "vt" lines, all "v" lines, all faces ...).
// A 1536^2 textured OBJ is 450 MB of shortest-round-trip decimals, 0.59 s single-threaded beside a 26 ms
// forward pass; the items are independent, so chunks of 32 Ki items are formatted by up to 12 host threads
// into their own strings and copied into the file with pwrite at the offsets the sizes give (0.23 s): the
// bytes are those of the sequential loop.
void write_section(FileSink& w, const FileSection& s) {
    constexpr int64_t kChunk = 32768;
    const int64_t count = s.count, nchunks = (count + kChunk - 1) / kChunk;
    unsigned hw = std::thread::hardware_concurrency();
    const int nthreads = s.threads ? (int)std::min<int64_t>(nchunks, hw ? (hw > 12 ? 12 : hw) : 4) : 1;
    if (nthreads <= 1) {
        for (int64_t i = 0; i < count; ++i) {
            w.flush_if_full();
            s.item(s.args, i, w.buf);
        }
        return;
    }
    w.flush();
    std::vector<std::string> chunks((size_t)nchunks);
    for_each_chunk(nchunks, nthreads, [&](int64_t c) {
        std::string& out = chunks[(size_t)c];
        out.reserve(1 << 20);
        const int64_t end = std::min(count, (c + 1) * kChunk);
        for (int64_t i = c * kChunk; i < end; ++i) s.item(s.args, i, out);
        return 0;
    });
    // the same threads then copy their chunks into the file at the offsets the sizes give
    ME_CHECK(fflush(w.f) == 0, ME_ERR_IO, "write failed: %s", strerror(errno));
    const off_t base = ftello(w.f);
    std::vector<off_t> offset((size_t)nchunks + 1, base);
    for (int64_t c = 0; c < nchunks; ++c) offset[(size_t)c + 1] = offset[(size_t)c] + (off_t)chunks[(size_t)c].size();
    const int fd = fileno(w.f);
    const int failed = for_each_chunk(nchunks, nthreads, [&](int64_t c) {
        const int e = pwrite_all(fd, chunks[(size_t)c].data(), chunks[(size_t)c].size(), offset[(size_t)c]);
        if (!e) std::string().swap(chunks[(size_t)c]);
        return e;
    });
    ME_CHECK(failed == 0, ME_ERR_IO, "write failed: %s", strerror(failed));
    ME_CHECK(fseeko(w.f, offset[(size_t)nchunks], SEEK_SET) == 0, ME_ERR_IO, "seek failed: %s", strerror(errno));
}

}  // namespace

void write_sections(const std::string& path, const std::string& head, const FileSection* sections, int count) {
    FileSink w(path);
    w.buf += head;
    for (int k = 0; k < count; ++k) write_section(w, sections[k]);
    w.close();
}

// `bytes` into a new file: chunks of 8 MiB (page-cache copies scale with threads; one thread moves ~2 GB/s)
void write_bytes_parallel(const std::string& path, const char* data, size_t bytes) {
    FILE* f = fopen(path.c_str(), "wb");
    ME_CHECK(f, ME_ERR_IO, "cannot create %s: %s", path.c_str(), strerror(errno));
    const int fd = fileno(f);
    constexpr size_t kChunk = 8u << 20;
    const int64_t nchunks = (int64_t)((bytes + kChunk - 1) / kChunk);
    // Two threads: the copy into the page cache runs at 2.4 - 2.7 GB/s per FILE with 2 or with 8 writers, and with one
    // rank per GPU writing at once eight writers per file cost the node half of what it can take (tools/
    // node_write_ceiling.py on the 256-core host: 8 processes x 2 threads 20.6 GB/s, x 8 threads 9.7 GB/s).  ME_WRITE_THREADS.
    static const int want = std::max(1, std::min(64, env_int("ME_WRITE_THREADS", 2)));
    const int failed = for_each_chunk(nchunks, (int)std::min<int64_t>(nchunks, want), [&](int64_t c) {
        const size_t at = (size_t)c * kChunk;
        return pwrite_all(fd, data + at, std::min(bytes - at, kChunk), (off_t)at);
    });
    const int r = fclose(f);
    ME_CHECK(failed == 0, ME_ERR_IO, "write failed: %s", strerror(failed));
    ME_CHECK(r == 0, ME_ERR_IO, "close failed: %s", strerror(errno));
}

// pinned staging buffer of write slot `which` (the D2H copy of a few hundred MB runs at the link rate only from pinned
// memory), grown in 64 MiB steps
char* pinned_buf(me_ctx* ctx, size_t bytes, int which) {
    me_ctx::WriteSlot& w = ctx->write_slots[(size_t)which];
    if (w.pinned && w.pinned_bytes >= bytes) return (char*)w.pinned;
    if (w.pinned) ME_HIP(hipHostFree(w.pinned));
    w.pinned = nullptr, w.pinned_bytes = 0;
    const size_t want = grow_in_steps(bytes);
    ME_HIP(hipHostMalloc(&w.pinned, want, hipHostMallocDefault));
    w.pinned_bytes = want;
    return (char*)w.pinned;
}

// waits for pending write k; a failure becomes the Error of the caller that waited for it
void join_pending_write(me_ctx* ctx, int k) {
    me_ctx::WriteSlot& w = ctx->write_slots[(size_t)k];
    if (!w.active) return;
    if (w.th.joinable()) w.th.join();
    w.active = false;
    if (w.code) {
        const int32_t code = w.code;
        const std::string msg = w.msg;
        w.code = 0, w.msg.clear();
        fail(code, "write-behind: %s", msg.c_str());
    }
}

void write_pinned_file(me_ctx* ctx, const PinnedFile& file, bool behind) {
    const auto write = [](const PinnedFile& f) {
        write_bytes_parallel(f.dest, f.data, f.bytes);
        if (!f.side_path.empty()) write_sections(f.side_path, f.side_text, nullptr, 0);
    };
    if (!behind) return write(file);
    me_ctx::WriteSlot& w = ctx->write_slots[(size_t)file.slot];
    w.active = true, w.code = 0, w.msg.clear(), w.dest = file.dest;
    w.th = std::thread([&w, file, write]() {
        try {
            write(file);
        } catch (const me::Error& e) {
            w.code = e.code, w.msg = e.msg;
        } catch (const std::exception& e) {
            w.code = ME_ERR_IO, w.msg = e.what();
        }
    });
}

}  // namespace me

using namespace me;

extern "C" int32_t me_ctx_set_write_behind(me_ctx* ctx, int32_t files_in_flight) {
    if (!ctx || files_in_flight < 0 || files_in_flight > 64) return ME_ERR_BAD_ARG;
    const int32_t rc = me_output_flush(ctx);  // nothing in flight while the slots change
    const int n = files_in_flight == 0 ? 0 : (files_in_flight < 2 ? 2 : files_in_flight);
    (void)hipSetDevice(ctx->device);
    for (size_t k = (size_t)(n > 1 ? n : 1); k < ctx->write_slots.size(); ++k)
        if (ctx->write_slots[k].pinned) (void)hipHostFree(ctx->write_slots[k].pinned);
    ctx->write_slots.resize((size_t)(n > 1 ? n : 1));
    ctx->write_behind = n;
    ctx->write_next = 0;
    return rc;
}

extern "C" int32_t me_output_flush(me_ctx* ctx) {
    if (!ctx) return ME_ERR_BAD_ARG;
    int32_t rc = ME_OK;
    // (output overlap: the output stream's queued kernels and copies too)
    if (ctx->output_overlap && ctx->out_stream && hipStreamSynchronize(ctx->out_stream) != hipSuccess)
        ctx->last_error = "me_output_flush: the output stream failed", rc = ME_ERR_HIP;
    for (int k = 0; k < (int)ctx->write_slots.size(); ++k) {
        try {
            join_pending_write(ctx, k);
        } catch (const me::Error& e) {
            if (rc == ME_OK) ctx->last_error = e.msg, rc = e.code;
        }
    }
    return rc;
}
