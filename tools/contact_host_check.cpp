// Stand-alone check of the contacts' host arithmetic (unmicst_amd/csrc/umx_contact_host.h): the limits, the first table size and the
// ordering of a scattered list, held to std::sort of the whole list.  No HIP, no GPU; meant to be built with the host sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/contact_host_check.cpp -o contact_host_check
// (tests/test_label_contacts_cpu.py does that and runs it).  Prints "contact-host-ok" and exits 0, or says what failed and exits 1.
#include <cstdint>
#include <cstring>
#include <random>
#include <vector>

#include "../unmicst_amd/csrc/umx_contact_host.h"

static int failures = 0;
#define EXPECT(cond)                                                       \
    do {                                                                   \
        if (!(cond)) { printf("line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

static bool refused(int H, int W, long long n, int reach, const char* word) {
    char buf[200];
    umx::contact_check_message(H, W, n, reach, buf, sizeof buf);
    return word ? strstr(buf, word) != nullptr : buf[0] == 0;
}

int main() {
    EXPECT(refused(1, 1, 0, 0, nullptr) && refused(1, INT_MAX, INT_MAX, 255, nullptr) && refused(46340, 46340, 5, 1, nullptr));
    EXPECT(refused(0, 1, 0, 0, "at least 1") && refused(1, 0, 0, 0, "at least 1") && refused(-3, 4, 0, 0, "at least 1"));
    EXPECT(refused(2, 1 << 30, 0, 0, "flat pixel index") && refused(65536, 65536, 0, 0, "flat pixel index"));
    EXPECT(refused(4, 4, -1, 0, "n_objects") && refused(4, 4, (long long)INT_MAX + 1, 0, "n_objects"));
    EXPECT(refused(4, 4, 1, -1, "reach") && refused(4, 4, 1, 256, "reach"));
    char tiny[8];
    umx::contact_check_message(0, 0, 0, 0, tiny, sizeof tiny);   // a message longer than its buffer is cut, not overrun
    EXPECT(strlen(tiny) == sizeof tiny - 1);
    umx::contact_check_message(0, 0, 0, 0, nullptr, 0);

    EXPECT(umx::contact_first_table(0) == UMX_CONTACT_TABLE_MIN && umx::contact_first_table(UMX_CONTACT_TABLE_MIN) == UMX_CONTACT_TABLE_MIN);
    EXPECT(umx::contact_first_table(UMX_CONTACT_TABLE_MIN + 1) == 2 * (size_t)UMX_CONTACT_TABLE_MIN);
    EXPECT(umx::contact_first_table(157501) == 262144 && umx::contact_first_table(INT_MAX) == (size_t)UMX_CONTACT_TABLE_MAX);

    // rows in order of a, every row shuffled: a hub of 20 000 contacts, rows of one, labels without a row
    std::mt19937 rng(5);
    std::vector<umx_label_contact> list;
    auto row = [&](int a, int n) {
        std::vector<int> bs(n);
        for (int k = 0; k < n; ++k) bs[k] = a + 1 + 3 * k;
        std::shuffle(bs.begin(), bs.end(), rng);
        for (int b : bs) list.push_back(umx_label_contact{a, b, (uint32_t)a + (uint32_t)b, 0});
    };
    row(1, 20000); row(2, 1); row(3, 1); row(7, 64); row(9, 2); row(INT_MAX - 400, 100);
    std::vector<umx_label_contact> want = list;
    std::sort(want.begin(), want.end(), [](const umx_label_contact& x, const umx_label_contact& y) { return x.a != y.a ? x.a < y.a : x.b < y.b; });
    EXPECT(umx::contact_sort_rows(list.data(), (long long)list.size()) == 20000);
    EXPECT(memcmp(list.data(), want.data(), list.size() * sizeof(umx_label_contact)) == 0);
    EXPECT(umx::contact_sort_rows(list.data(), 0) == 0 && umx::contact_sort_rows(nullptr, 0) == 0);
    EXPECT(umx::contact_sort_rows(list.data(), 1) == 1);

    if (failures) return 1;
    printf("contact-host-ok\n");
    return 0;
}
