// Host twin of the device weight packer (csrc/weight_pack.hip) and the checks of the arena cache header: csrc/weight_pack.h
// compiled as plain C++ (ME_PACK_HOST).
//   weight_pack_host pack <dtype> <kind> <dup> <src_dtype> <ndim> <d0> .. <src.bin> <host.bin> <lanes.bin>
//       host.bin: the host packer (pack_host).  lanes.bin: the kernels' work, lane by lane -- the destination-major index map
//       for the flat kernels, and for the two transposing kernels every workgroup's load phase into an LDS tile and its
//       store phase out of it, with every index checked against its array.  Destination elements no lane wrote keep 0xAA.
//   weight_pack_host header      round trip and every damaged / stale form of the cache header; prints one line per check
//   weight_pack_host path <checkpoint> <dtype name> <layout hex>
#define ME_PACK_HOST
#include "../matrix-eyes_amd/csrc/weight_pack.h"

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

using namespace me_pack;

static std::vector<char> read_file(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) {
        fprintf(stderr, "cannot open %s\n", path);
        exit(2);
    }
    std::vector<char> out;
    char buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) out.insert(out.end(), buf, buf + n);
    fclose(f);
    return out;
}

static void write_file(const char* path, const std::vector<char>& data) {
    FILE* f = fopen(path, "wb");
    if (!f || fwrite(data.data(), 1, data.size(), f) != data.size()) {
        fprintf(stderr, "cannot write %s\n", path);
        exit(2);
    }
    fclose(f);
}

#define REQUIRE(cond)                                                       \
    do {                                                                    \
        if (!(cond)) {                                                      \
            fprintf(stderr, "%s:%d: %s does not hold\n", __FILE__, __LINE__, #cond); \
            exit(3);                                                        \
        }                                                                   \
    } while (0)

static void lanes(const Shape& s, int32_t dtype, const void* src, int32_t src_dtype, std::vector<char>& out) {
    const bool f32 = s.kind == K_VEC_F32 || s.kind == K_CONVK_F32;
    uint16_t* o16 = reinterpret_cast<uint16_t*>(out.data());
    uint32_t* o32 = reinterpret_cast<uint32_t*>(out.data());
    if (s.kind == K_CONV_16 || s.kind == K_CONVT_16) {
        const bool conv = s.kind == K_CONV_16;
        const int64_t gx = (s.Cin + kTileCi - 1) / kTileCi, gy = conv ? s.Cout : (s.Cout + kTileCo - 1) / kTileCo;
        const int elems = conv ? kConvTileElems : kConvtTileElems;
        std::vector<uint16_t> tile((size_t)elems);
        std::vector<char> written((size_t)elems);
        for (int64_t by = 0; by < gy; ++by)
            for (int64_t bx = 0; bx < gx; ++bx) {
                std::fill(written.begin(), written.end(), 0);
                const int nl = conv ? conv_tile_loads(s, bx) : convt_tile_loads(s, bx, by);
                for (int t = 0; t < kTileThreads; ++t)
                    for (int i = t; i < nl; i += kTileThreads) {
                        const TileRef r = conv ? conv_tile_load(s, bx, by, i) : convt_tile_load(s, bx, by, i);
                        REQUIRE(r.lds >= 0 && r.lds < elems && r.g >= 0 && r.g < s.numel);
                        tile[(size_t)r.lds] = src_get16(src, src_dtype, r.g, dtype);
                        written[(size_t)r.lds] = 1;
                    }
                const int ns = conv ? conv_tile_stores(s) : convt_tile_stores(s, by);
                if (tile_store8_ok(s)) {   // the 16-byte form: eight channels per work item
                    for (int t = 0; t < kTileThreads; ++t)
                        for (int i = t; i < ns / 8; i += kTileThreads) {
                            TileRef r;
                            const int item = tile_store8_item(i);
                            if (!(conv ? conv_tile_store(s, bx, by, item, &r) : convt_tile_store(s, bx, by, item, &r))) continue;
                            REQUIRE(r.lds % 2 == 0 && r.g % 8 == 0 && r.lds >= 0 && r.lds + 8 <= elems && r.g >= 0 && r.g + 8 <= s.dst_elems);
                            for (int j = 0; j < 8; ++j) {
                                REQUIRE(written[(size_t)r.lds + j]);
                                o16[r.g + j] = tile[(size_t)r.lds + j];
                            }
                        }
                    continue;
                }
                for (int t = 0; t < kTileThreads; ++t)
                    for (int i = t; i < ns; i += kTileThreads) {
                        TileRef r;
                        if (!(conv ? conv_tile_store(s, bx, by, i, &r) : convt_tile_store(s, bx, by, i, &r))) continue;
                        REQUIRE(r.lds >= 0 && r.lds < elems && written[(size_t)r.lds] && r.g >= 0 && r.g < s.dst_elems);
                        o16[r.g] = tile[(size_t)r.lds];
                    }
            }
        return;
    }
    for (int64_t d = 0; d < s.dst_elems; ++d) {
        const int64_t si = src_index(s, d);
        REQUIRE(si >= 0 && si < s.numel);
        if (f32)
            o32[d] = src_get32(src, src_dtype, si);
        else
            o16[d] = src_get16(src, src_dtype, si, dtype);
    }
}

static int cmd_pack(int argc, char** argv) {
    if (argc < 7) return 2;
    const int32_t dtype = atoi(argv[2]), kind = atoi(argv[3]), dup = atoi(argv[4]), src_dtype = atoi(argv[5]), ndim = atoi(argv[6]);
    if (ndim < 1 || ndim > 4 || argc != 7 + ndim + 3) return 2;
    int64_t dims[4] = {1, 1, 1, 1};
    for (int i = 0; i < ndim; ++i) dims[i] = atoll(argv[7 + i]);
    Shape s;
    if (const char* why = make_shape(kind, dup, dims, ndim, &s)) {
        fprintf(stderr, "%s\n", why);
        return 4;
    }
    const std::vector<char> src = read_file(argv[7 + ndim]);
    REQUIRE(src.size() == (size_t)s.numel * src_elem_size(src_dtype));
    std::vector<char> host((size_t)s.dst_bytes, (char)0xAA), lane((size_t)s.dst_bytes, (char)0xAA);
    pack_host(s, dtype, src.data(), src_dtype, host.data());
    lanes(s, dtype, src.data(), src_dtype, lane);
    write_file(argv[7 + ndim + 1], host);
    write_file(argv[7 + ndim + 2], lane);
    return 0;
}

static int cmd_header() {
    ArenaExpect e;
    e.dtype = 1, e.split_mask = 3, e.layout = 0x0123456789abcdefull, e.arena_bytes = 1024;
    for (int i = 0; i < kArenaConfigWords; ++i) e.config[i] = 100u + (uint32_t)i;
    std::vector<char> file(kArenaHeaderBytes + 1024, 0);
    arena_header_write(e, 777, 123456789012345ll, 0xfeedull, file.data());
    ArenaHeader h;
    int bad = 0;
    auto expect = [&](const char* what, ArenaVerdict got, ArenaVerdict want) {
        printf("%s: %s (%d)\n", what, arena_verdict_text(got), (int)got);
        if (got != want) ++bad;
    };
    auto check = [&](const std::vector<char>& f, size_t have, uint64_t file_bytes, const ArenaExpect& ex, bool has_source, int64_t size,
                     int64_t mtime) { return arena_header_check(f.data(), have, file_bytes, ex, has_source, size, mtime, &h); };
    expect("round trip", check(file, file.size(), file.size(), e, true, 777, 123456789012345ll), ARENA_OK);
    if (h.checksum != 0xfeedull || h.layout != e.layout || h.source_size != 777 || h.format != ME_ARENA_FORMAT) ++bad;
    expect("checkpoint absent", check(file, file.size(), file.size(), e, false, -1, -1), ARENA_OK);
    expect("another size", check(file, file.size(), file.size(), e, true, 778, 123456789012345ll), ARENA_STALE_SOURCE);
    expect("another mtime", check(file, file.size(), file.size(), e, true, 777, 123456789012346ll), ARENA_STALE_SOURCE);
    expect("short header", check(file, 100, 100, e, true, 777, 123456789012345ll), ARENA_SHORT);
    expect("truncated payload", check(file, kArenaHeaderBytes, file.size() - 1, e, true, 777, 123456789012345ll), ARENA_SHORT);
    expect("trailing bytes", check(file, kArenaHeaderBytes, file.size() + 1, e, true, 777, 123456789012345ll), ARENA_BAD_SIZE);
    {
        std::vector<char> f = file;
        f[0] ^= 1;
        expect("wrong magic", check(f, f.size(), f.size(), e, true, 777, 123456789012345ll), ARENA_BAD_MAGIC);
    }
    {
        std::vector<char> f = file;
        const uint32_t other = ME_ARENA_FORMAT + 1;
        memcpy(f.data() + 8, &other, 4);
        expect("another format constant", check(f, f.size(), f.size(), e, true, 777, 123456789012345ll), ARENA_STALE_FORMAT);
    }
    {
        std::vector<char> f = file;
        const uint32_t other = 128;
        memcpy(f.data() + 12, &other, 4);
        expect("another header size", check(f, f.size(), f.size(), e, true, 777, 123456789012345ll), ARENA_BAD_HEADER);
    }
    {
        ArenaExpect o = e;
        o.layout ^= 1;
        expect("another layout hash", check(file, file.size(), file.size(), o, true, 777, 123456789012345ll), ARENA_OTHER_CONTEXT);
        o = e, o.arena_bytes = 2048;
        expect("another arena size", check(file, file.size(), file.size(), o, true, 777, 123456789012345ll), ARENA_OTHER_CONTEXT);
        o = e, o.split_mask = 0;
        expect("another split mask", check(file, file.size(), file.size(), o, true, 777, 123456789012345ll), ARENA_OTHER_CONTEXT);
        o = e, o.dtype = 0;
        expect("another dtype", check(file, file.size(), file.size(), o, true, 777, 123456789012345ll), ARENA_OTHER_CONTEXT);
        o = e, o.config[16] ^= 1;
        expect("another configuration", check(file, file.size(), file.size(), o, true, 777, 123456789012345ll), ARENA_OTHER_CONTEXT);
    }
    // the checksum: any order of the terms, one changed word changes it
    uint64_t fwd = 0, rev = 0, flipped = 0;
    const uint32_t words[5] = {0, 1, 0xffffffffu, 0, 12345};
    for (int i = 0; i < 5; ++i) fwd += checksum_term((uint64_t)i, words[i]);
    for (int i = 4; i >= 0; --i) rev += checksum_term((uint64_t)i, words[i]);
    for (int i = 0; i < 5; ++i) flipped += checksum_term((uint64_t)i, i == 3 ? 1u : words[i]);
    printf("checksum: %s\n", fwd == rev && fwd != flipped && checksum_term(0, 0) != checksum_term(1, 0) ? "ok" : "WRONG");
    if (!(fwd == rev && fwd != flipped && checksum_term(0, 0) != checksum_term(1, 0))) ++bad;
    return bad ? 5 : 0;
}

static int cmd_path(int argc, char** argv) {
    if (argc != 5) return 2;
    char buf[4096];
    const int64_t n = arena_cache_path(argv[2], argv[3], strtoull(argv[4], nullptr, 16), buf, sizeof buf);
    if (n < 0) return 4;
    char tiny[8];
    REQUIRE(arena_cache_path(argv[2], argv[3], 0, tiny, sizeof tiny) == -1);
    printf("%s\n", buf);
    return (size_t)n == strlen(buf) ? 0 : 5;
}

int main(int argc, char** argv) {
    const std::string cmd = argc > 1 ? argv[1] : "";
    if (cmd == "pack") return cmd_pack(argc, argv);
    if (cmd == "header") return cmd_header();
    if (cmd == "path") return cmd_path(argc, argv);
    fprintf(stderr, "usage: weight_pack_host pack|header|path ...\n");
    return 2;
}
