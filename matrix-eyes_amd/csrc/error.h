// How the library refuses: me::Error, thrown by me::fail and turned into a status code at the C ABI.  Free of HIP, so that the headers
// a host compiler builds alone (gemm_params.h, admission.h) can raise exactly what the .hip side raises.
#pragma once
#include <stdint.h>
#include <string>

namespace me {

// Thrown inside the library, caught at the C ABI; nothing escapes to the caller.
struct Error {
    int32_t code;
    std::string msg;
};

// (one definition in the library: gemm.hip; a host test program brings its own)
[[noreturn]] void fail(int32_t code, const char* fmt, ...);

#define ME_CHECK(cond, code, ...)                   \
    do {                                            \
        if (!(cond)) ::me::fail((code), __VA_ARGS__); \
    } while (0)

}  // namespace me
