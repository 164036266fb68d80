// Stand-alone check of the relabel's host part (unmicst_amd/csrc/umx_relabel_host.h): the limits of a call, the validation of keep and
// pairs, and the union-find that numbers the classes, at the ends of their ranges.  No HIP, no GPU; meant to be built with the host
// sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/relabel_host_check.cpp -o relabel_host_check
// (tests/test_label_relabel_cpu.py does that and runs it).  Prints "relabel-host-ok" and exits 0, or says what failed and exits 1.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../unmicst_amd/csrc/umx_relabel_host.h"

static int failures = 0;
#define EXPECT(cond)                                                       \
    do {                                                                   \
        if (!(cond)) { printf("line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

// word != null: the call is refused with a message that holds it; null: it is accepted
static bool refused(int H, int W, long long n, long long m, const char* word) {
    char buf[240];
    umx::relabel_check_message(H, W, n, m, buf, sizeof buf);
    return word ? strstr(buf, word) != nullptr : buf[0] == 0;
}

struct Result {
    int rc;
    long long n_new;
    std::vector<int32_t> map;
    char msg[240];
};

static Result run(long long N, const std::vector<uint8_t>* keep, const std::vector<int32_t>& pairs) {
    Result r;
    r.map.assign((size_t)N + 1, -7);
    r.n_new = -1;
    r.msg[0] = 0;
    r.rc = umx::relabel_map(N, keep ? keep->data() : nullptr, pairs.empty() ? nullptr : pairs.data(), (long long)pairs.size() / 2, r.map.data(),
                            &r.n_new, r.msg, sizeof r.msg);
    return r;
}

int main() {
    // the limits
    EXPECT(refused(1, 1, 0, 0, nullptr) && refused(32767, 65536, INT_MAX - 1, UMX_RELABEL_MAX_PAIRS, nullptr) && refused(1, INT_MAX, 5, 5, nullptr));
    EXPECT(refused(0, 1, 0, 0, "at least 1") && refused(1, 0, 0, 0, "at least 1") && refused(-3, 4, 0, 0, "at least 1"));
    EXPECT(refused(32768, 65536, 0, 0, "flat pixel index") && refused(46341, 46341, 0, 0, "flat pixel index") && refused(2, INT_MAX, 0, 0, "flat pixel index"));
    EXPECT(refused(4, 4, -1, 0, "n_objects") && refused(4, 4, INT_MAX, 0, "n_objects") && refused(4, 4, INT64_MIN, 0, "n_objects") &&
           refused(4, 4, INT64_MAX, 0, "n_objects"));
    EXPECT(refused(4, 4, 0, -1, "n_pairs") && refused(4, 4, 0, (long long)UMX_RELABEL_MAX_PAIRS + 1, "n_pairs") && refused(4, 4, 0, INT64_MAX, "n_pairs"));
    char tiny[8];
    umx::relabel_check_message(0, 0, 0, 0, tiny, sizeof tiny);      // a message longer than its buffer is cut, not overrun
    EXPECT(strlen(tiny) == sizeof tiny - 1);
    umx::relabel_check_message(0, 0, 0, 0, nullptr, 0);

    // N = 0: the map is its one word
    {
        Result r = run(0, nullptr, {});
        EXPECT(r.rc == UMX_OK && r.n_new == 0 && r.map.size() == 1 && r.map[0] == 0);
        std::vector<uint8_t> none;
        r = run(0, &none, {});
        EXPECT(r.rc == UMX_OK && r.n_new == 0 && r.map[0] == 0);
        r = run(0, nullptr, {1, 1});
        EXPECT(r.rc == UMX_ERR_INVALID && strstr(r.msg, "pair 0"));
    }
    // the identity, keep null and keep all ones
    {
        const long long N = 4097;
        std::vector<uint8_t> all((size_t)N, 1);
        for (const std::vector<uint8_t>* keep : {(const std::vector<uint8_t>*)nullptr, (const std::vector<uint8_t>*)&all}) {
            Result r = run(N, keep, {});
            bool same = r.rc == UMX_OK && r.n_new == N;
            for (long long j = 0; j <= N; ++j) same = same && r.map[(size_t)j] == j;
            EXPECT(same);
        }
    }
    // the chain (1,2),(2,3),...,(N-1,N), ascending and descending: one class; with every second label dropped first: refused at pair 0
    {
        const long long N = 1 << 20;
        std::vector<int32_t> up, down;
        for (int32_t j = 1; j < N; ++j) { up.push_back(j); up.push_back(j + 1); }
        for (int32_t j = (int32_t)N; j > 1; --j) { down.push_back(j); down.push_back(j - 1); }
        for (const std::vector<int32_t>* p : {&up, &down}) {
            Result r = run(N, nullptr, *p);
            bool one = r.rc == UMX_OK && r.n_new == 1 && r.map[0] == 0;
            for (long long j = 1; j <= N; ++j) one = one && r.map[(size_t)j] == 1;
            EXPECT(one);
        }
        std::vector<uint8_t> keep((size_t)N, 1);
        keep[1] = 0;
        Result r = run(N, &keep, up);
        EXPECT(r.rc == UMX_ERR_INVALID && strstr(r.msg, "pair 0") && strstr(r.msg, "label 2"));
    }
    // a star round the LAST label, with duplicates, (a, a) and (b, a); two labels stay alone, one of them dropped
    {
        const long long N = 1000;
        std::vector<int32_t> p;
        for (int32_t j = 3; j < N; ++j) { p.push_back((int32_t)N); p.push_back(j); p.push_back(j); p.push_back((int32_t)N); p.push_back(j); p.push_back(j); }
        std::vector<uint8_t> keep((size_t)N, 1);
        keep[0] = 0;
        Result r = run(N, &keep, p);
        bool ok = r.rc == UMX_OK && r.n_new == 2 && r.map[0] == 0 && r.map[1] == 0 && r.map[2] == 1;
        for (long long j = 3; j <= N; ++j) ok = ok && r.map[(size_t)j] == 2;
        EXPECT(ok);
    }
    // a refused pair at every position: out of range on either side, or a dropped label
    {
        const long long N = 50;
        std::vector<uint8_t> keep((size_t)N, 1);
        keep[9] = 0;
        std::vector<int32_t> good;
        for (int32_t j = 20; j < 40; ++j) { good.push_back(j); good.push_back(j + 1); }
        const int32_t bad[][2] = {{0, 5}, {5, 0}, {-1, 5}, {5, (int32_t)N + 1}, {INT_MAX, 5}, {INT_MIN, 5}, {10, 5}, {5, 10}, {10, 10}};
        for (const auto& b : bad) {
            for (size_t at = 0; at <= good.size() / 2; ++at) {
                std::vector<int32_t> p = good;
                p.insert(p.begin() + 2 * (long)at, {b[0], b[1]});
                Result r = run(N, &keep, p);
                char want[32];
                snprintf(want, sizeof want, "pair %zu is", at);
                EXPECT(r.rc == UMX_ERR_INVALID && strstr(r.msg, want));
            }
        }
        EXPECT(run(N, &keep, good).rc == UMX_OK && run(N, &keep, good).n_new == N - 1 - 20);
        EXPECT(umx::relabel_map(N, nullptr, nullptr, 3, nullptr, nullptr, nullptr, 0) == UMX_ERR_INVALID);   // pairs null with M > 0
    }
    // N at the limit of the 32-bit index arithmetic, validation only: no map, no keep, nothing of size N is touched
    {
        const long long N = umx::kRelabelMaxObjects;
        const std::vector<int32_t> p = {1, (int32_t)N, (int32_t)N, (int32_t)N - 1};
        char msg[240];
        long long n_new = -5;
        EXPECT(umx::relabel_map(N, nullptr, p.data(), 2, nullptr, &n_new, msg, sizeof msg) == UMX_OK && n_new == -5 && msg[0] == 0);
        const std::vector<int32_t> q = {1, (int32_t)N, INT_MAX, 1};
        EXPECT(umx::relabel_map(N, nullptr, q.data(), 2, nullptr, &n_new, msg, sizeof msg) == UMX_ERR_INVALID && strstr(msg, "pair 1 is"));
        EXPECT(umx::relabel_map(N + 1, nullptr, nullptr, 0, nullptr, nullptr, msg, sizeof msg) == UMX_ERR_INVALID && strstr(msg, "n_objects"));
        EXPECT(umx::relabel_map(N, nullptr, nullptr, (long long)UMX_RELABEL_MAX_PAIRS + 1, nullptr, nullptr, msg, sizeof msg) == UMX_ERR_INVALID &&
               strstr(msg, "n_pairs"));
        umx::relabel_map(-1, nullptr, nullptr, 0, nullptr, nullptr, tiny, sizeof tiny);
        EXPECT(strlen(tiny) == sizeof tiny - 1);
    }
    static_assert(sizeof(size_t) == 8, "sizes are 64 bits");

    if (failures) return 1;
    printf("relabel-host-ok\n");
    return 0;
}
