// Stand-alone check of the hulls' host arithmetic (unmicst_amd/csrc/umx_hull_host.h): the limits of a call, the limit on E and the
// sizes of the buffers E and N give, at the ends of their ranges.  No HIP, no GPU; meant to be built with the host sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/hull_host_check.cpp -o hull_host_check
// (tests/test_label_hull_cpu.py does that and runs it).  Prints "hull-host-ok" and exits 0, or says what failed and exits 1.
#include <cstdint>
#include <cstring>

#include "../unmicst_amd/csrc/umx_hull_host.h"

static int failures = 0;
#define EXPECT(cond)                                                       \
    do {                                                                   \
        if (!(cond)) { printf("line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

// word != null: the call is refused with a message that holds it; null: it is accepted
static bool refused(int H, int W, long long n, const char* word) {
    char buf[240];
    umx::hull_check_message(H, W, n, buf, sizeof buf);
    return word ? strstr(buf, word) != nullptr : buf[0] == 0;
}

static bool rows_refused(long long E, long long n, int H, const char* word) {
    char buf[240];
    umx::hull_rows_message(E, n, H, buf, sizeof buf);
    return word ? strstr(buf, word) != nullptr : buf[0] == 0;
}

int main() {
    EXPECT(refused(1, 1, 0, nullptr) && refused(65536, 8, INT_MAX, nullptr) && refused(4, 65536, 5, nullptr) && refused(46340, 46340, 5, nullptr));
    EXPECT(refused(32767, 65536, 0, nullptr) && refused(32768, 65536, 0, "flat pixel index") && refused(65536, 65536, 0, "flat pixel index"));
    EXPECT(refused(0, 1, 0, "at least 1") && refused(1, 0, 0, "at least 1") && refused(-3, 4, 0, "at least 1"));
    EXPECT(refused(65537, 1, 0, "at most 65536") && refused(1, 65537, 0, "at most 65536") && refused(1, INT_MAX, 0, "at most 65536"));
    EXPECT(refused(4, 4, -1, "n_objects") && refused(4, 4, (long long)INT_MAX + 1, "n_objects") && refused(4, 4, INT64_MIN, "n_objects"));
    char tiny[8];
    umx::hull_check_message(0, 0, 0, tiny, sizeof tiny);            // a message longer than its buffer is cut, not overrun
    EXPECT(strlen(tiny) == sizeof tiny - 1);
    umx::hull_check_message(0, 0, 0, nullptr, 0);
    umx::hull_rows_message(-1, 1, 1, tiny, sizeof tiny);
    EXPECT(strlen(tiny) == sizeof tiny - 1);
    umx::hull_rows_message(-1, 1, 1, nullptr, 0);

    // E: 0 .. N * H is what labels can give; above UMX_HULL_MAX_ROWS is too much; the largest N * H is below 2^47
    EXPECT(rows_refused(0, 0, 1, nullptr) && rows_refused(0, 5, 7, nullptr) && rows_refused(35, 5, 7, nullptr));
    EXPECT(rows_refused(36, 5, 7, "summed") && rows_refused(-1, 5, 7, "summed") && rows_refused(1, 0, 7, "summed"));
    EXPECT(rows_refused(UMX_HULL_MAX_ROWS, INT_MAX, 65536, nullptr) && rows_refused((long long)UMX_HULL_MAX_ROWS + 1, INT_MAX, 65536, "UMX_HULL_MAX_ROWS"));
    EXPECT(rows_refused(16385ll * 16384, 16384, 16385, "far-apart") && rows_refused(16384ll * 16384, 16384, 16385, nullptr));
    EXPECT(rows_refused((long long)INT_MAX * 65536, INT_MAX, 65536, "UMX_HULL_MAX_ROWS") && rows_refused((long long)INT_MAX * 65536 + 1, INT_MAX, 65536, "summed"));
    EXPECT(rows_refused(INT64_MAX, INT_MAX, 65536, "summed") && rows_refused(INT64_MIN, INT_MAX, 65536, "summed"));

    // the sizes, at both ends
    EXPECT(umx::hull_label_blocks(0, 2048) == 0 && umx::hull_label_blocks(1, 2048) == 1 && umx::hull_label_blocks(2048, 2048) == 1);
    EXPECT(umx::hull_label_blocks(2049, 2048) == 2 && umx::hull_label_blocks(INT_MAX, 2048) == (size_t)1 << 20);
    EXPECT(umx::hull_row_words(0) == 0 && umx::hull_row_words(UMX_HULL_MAX_ROWS) == (size_t)1 << 29);
    EXPECT(umx::hull_scratch_vertices(0, 0) == 0 && umx::hull_scratch_vertices(1, 1) == 4);                 // one pixel: 2 * 1 + 2 vertices
    EXPECT(umx::hull_scratch_vertices(UMX_HULL_MAX_ROWS, INT_MAX) == ((size_t)1 << 29) + ((size_t)1 << 32) - 2);
    EXPECT(umx::hull_scratch_vertices(UMX_HULL_MAX_ROWS, INT_MAX) * sizeof(umx_label_hull_vertex) / sizeof(umx_label_hull_vertex) ==
           umx::hull_scratch_vertices(UMX_HULL_MAX_ROWS, INT_MAX));                                          // (its bytes fit a size_t)
    EXPECT(umx::hull_offset_words(0, 2048, 2) == 2 && umx::hull_offset_words(157501, 2048, 2) == 157501 + 77 + 2);
    EXPECT(umx::hull_offset_words(INT_MAX, 2048, 2) == (size_t)INT_MAX + ((size_t)1 << 20) + 2);
    static_assert(sizeof(umx_label_hull) == 32 && sizeof(umx_label_hull_vertex) == 8, "the records");
    static_assert(sizeof(size_t) == 8, "sizes are 64 bits");

    if (failures) return 1;
    printf("hull-host-ok\n");
    return 0;
}
