// Prints what image_groups (gator_amd/csrc/image_groups.h) makes of every case given on the command line, one line per case.  A case is
// "N/i0,i1,..." (image_index of M members into N images), "N/null/M" (image_index NULL) or either with "/noslot" appended (slot NULL).
// Built by tests/test_host_image_groups.py as plain C++17: the header needs no HIP.  Every array has exactly the size the header
// documents plus one guard entry, which must come back untouched.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "image_groups.h"

static void print_list(const char* name, const std::vector<int32_t>& v, size_t n) {
    printf(" %s=", name);
    for (size_t i = 0; i < n; ++i) printf("%s%d", i ? "," : "", v[i]);
}

int main(int argc, char** argv) {
    constexpr int32_t kGuard = -77;
    for (int i = 1; i < argc; ++i) {
        std::string s = argv[i];
        const bool noslot = s.size() > 7 && s.compare(s.size() - 7, 7, "/noslot") == 0;
        if (noslot) s.resize(s.size() - 7);
        const size_t cut = s.find('/');
        if (cut == std::string::npos) { fprintf(stderr, "bad case '%s'\n", argv[i]); return 2; }
        const int N = atoi(s.c_str());
        std::string rest = s.substr(cut + 1);
        std::vector<int32_t> index;
        const bool null = rest.compare(0, 5, "null/") == 0;
        int M = null ? atoi(rest.c_str() + 5) : 0;
        if (!null) {
            for (size_t at = 0; at <= rest.size();) {
                const size_t end = rest.find(',', at) == std::string::npos ? rest.size() : rest.find(',', at);
                index.push_back(atoi(rest.substr(at, end - at).c_str()));
                at = end + 1;
            }
            M = (int)index.size();
        }
        std::vector<int32_t> img_off(N + 2, kGuard), member_of(M + 1, kGuard), slot(M + 1, kGuard);
        const gator::ImageGroups g = gator::image_groups(null ? nullptr : index.data(), M, N, null ? nullptr : img_off.data(),
                                                         null ? nullptr : member_of.data(), null || noslot ? nullptr : slot.data());
        const bool guards = img_off[N + 1] == kGuard && member_of[M] == kGuard && slot[M] == kGuard;
        if (g.error == gator::ImageGroups::kOutside) {
            printf("error=outside at=%d value=%d", g.at, g.value);
        } else if (g.error == gator::ImageGroups::kNullTooMany) {
            printf("error=null_too_many");
        } else {
            printf("most=%d", g.most);
            if (!null) {
                print_list("img_off", img_off, N + 1);
                print_list("member_of", member_of, M);
                if (!noslot) print_list("slot", slot, M);
            }
        }
        printf(" guards=%s\n", guards ? "ok" : "OVERWRITTEN");
    }
    return 0;
}
