// Host driver of csrc/jpeg_entropy.h for tests/test_jpeg_entropy_cpu.py: the routines the kernels of csrc/jpeg_entropy.hip
// are made of, run thread by thread on the CPU in the kernels' order -- speculate, sync rounds (three rotating buffers),
// the segmented sums, write -- and compared coefficient by coefficient with the host decoder (decode_jpeg_coefficients).
//
//   jpeg_entropy_host <in.jpg> <bits per subsequence, 0: default> <threads per workgroup>
// prints one report line ("where=device reason=0 segments=.. subseqs=.. bits=.. rounds=.. upload_bytes=.. workgroups=..
// differ=.. stuffed=..") and one "segments:" line with the planner's byte ranges.
// exit 0: decoded here and equal to the host decoder's coefficients; 4: declined (the reason in the report), and then 0 / 3
// on the "host=" word say whether the host decoder takes the file; 1: decoded here but NOT what the host decoder says;
// 2: usage / I/O
#define ME_JPEG_HOST 1
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <vector>

#include "../matrix-eyes_amd/csrc/jpeg_entropy.h"

using namespace me_jpeg_entropy;

int main(int argc, char** argv) {
    if (argc != 4) {
        std::fprintf(stderr, "usage: jpeg_entropy_host <in.jpg> <subseq bits> <workgroup>\n");
        return 2;
    }
    int S = std::atoi(argv[2]);
    const int group = std::atoi(argv[3]);
    if (S == 0) S = kDefaultSubseqBits;
    if (S < kMinSubseqBits || S > kMaxSubseqBits || S % 32 || group < 1) return 2;
    std::ifstream in(argv[1], std::ios::binary);
    if (!in) return 2;
    const std::vector<uint8_t> file((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());

    // the yardstick, and whether the host decoder takes the file at all
    matrix_eyes::JpegCoefficients want;
    bool host_ok = true;
    std::string host_words;
    try {
        want = matrix_eyes::decode_jpeg_coefficients(file, "<jpeg>");
    } catch (const matrix_eyes::ImageError& e) {
        host_ok = false, host_words = e.what();
    }

    int reason = 0, rounds = 0, nseg = 0, nsub = 0;
    size_t upload = 0, stuffed = 0;
    long long differ = -1;
    matrix_eyes::JpegEntropyPlan plan;
    try {
        plan = matrix_eyes::plan_jpeg_entropy(file, "<jpeg>");
        reason = plan.reason;
    } catch (const matrix_eyes::ImageError&) {
        reason = matrix_eyes::kJpegDeclineHostError;
    }
    std::vector<int16_t> coef;
    if (reason == 0) {
        std::vector<uint32_t> buf(upload_capacity(plan, S));
        const Layout lay = prepare(plan, file.data(), S, buf.data());
        if (lay.total > buf.size()) return 2;
        upload = lay.total * 4, nseg = lay.nseg, nsub = lay.nsub;
        for (size_t j = 0; j < plan.seg_begin.size(); ++j)
            for (size_t p = plan.seg_begin[j]; p + 1 < plan.seg_end[j]; ++p) stuffed += file[p] == 0xff && file[p + 1] == 0x00;
        const Stream st = stream_of(buf.data(), lay);
        const EntropyTables& t = *st.tables;
        std::vector<uint64_t> states((size_t)nsub * 3);
        std::vector<Counts> counts((size_t)nsub), before((size_t)nsub);
        for (int i = 0; i < nsub; ++i) speculate_thread(t, st, i, states.data(), counts.data());
        const int max_rounds = max_sync_rounds(buf.data(), lay, S);
        int converged_at = 0;
        while (!converged_at && rounds < max_rounds) {
            ++rounds;
            const uint64_t* prev = rounds >= 2 ? &states[(size_t)((rounds - 2) % 3) * nsub] : nullptr;
            int changed = 0;
            for (int i = 0; i < nsub; ++i)
                changed += sync_thread(t, st, i, prev, &states[(size_t)((rounds - 1) % 3) * nsub], &states[(size_t)(rounds % 3) * nsub],
                                       counts.data());
            if (!changed) converged_at = rounds;
        }
        if (!converged_at) {
            reason = matrix_eyes::kJpegDeclineNoSync;
        } else {
            // jpeg_entropy_scan_kernel + jpeg_entropy_carry_kernel: exclusive sums that restart at every segment
            Counts run = {0, {0, 0, 0}};
            for (int i = 0; i < nsub; ++i) {
                if (st.seg_sub0[st.sub_seg[i]] == i) run = Counts{0, {0, 0, 0}};
                before[(size_t)i] = run;
                run.blocks += counts[(size_t)i].blocks;
                for (int c = 0; c < 3; ++c) run.dc[c] += counts[(size_t)i].dc[c];
            }
            coef.assign(plan.frame.total_coefs, 0);
            for (int i = 0; i < nsub; ++i) {
                const int err = write_thread(t, st, i, &states[(size_t)(rounds % 3) * nsub], before.data(), coef.data());
                if (err > reason) reason = err;
            }
        }
    }
    const bool device = reason == 0;
    if (device && host_ok) {
        differ = plan.frame.total_coefs == want.total_coefs ? 0 : 1;
        const int16_t* w = want.comps[0].coef;  // the components' coefficients are contiguous, in component order
        for (size_t i = 0; differ == 0 && i < coef.size(); ++i) differ += coef[i] != w[i];
    }
    std::printf("where=%s reason=%d segments=%d subseqs=%d bits=%d rounds=%d upload_bytes=%zu workgroups=%d differ=%lld stuffed=%zu host=%d\n",
                device ? "device" : "host", reason, nseg, nsub, S, rounds, upload, (nsub + group - 1) / group, differ, stuffed,
                host_ok ? 0 : 3);
    std::printf("segments:");
    for (size_t j = 0; j < plan.seg_begin.size(); ++j) std::printf(" %zu-%zu", plan.seg_begin[j], plan.seg_end[j]);
    std::printf("\nscan: %zu-%zu interval=%d why=%s\n", plan.scan_begin, plan.scan_end, plan.restart_interval, plan.why.c_str());
    if (!host_ok) std::fprintf(stderr, "%s\n", host_words.c_str());
    if (!device) return 4;
    return host_ok && differ == 0 ? 0 : 1;
}
