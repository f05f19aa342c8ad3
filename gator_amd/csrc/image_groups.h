// The grouping rule of the libraries whose members (meshes, people) are drawn into images (render.hip, draw2d.hip): plain C++, nothing of
// HIP, so that tests/host_image_groups.cpp builds it alone.  It reports an error as a value; the caller words the message.
#pragma once
#include <cstdint>

namespace gator {

struct ImageGroups {
    enum Error { kOk = 0, kOutside, kNullTooMany };
    Error error = kOk;
    int at = 0, value = 0;  // kOutside: the offending position and what stands there
    int32_t most = 0;       // the largest number of members in one image
};

// image_index[M] names the image, 0..N-1, of every member.  Fills img_off[N+1] (prefix counts), member_of[M] (the members of image n, in
// member order, at img_off[n]..) and, unless NULL, slot[M] (the rank of a member within its image).  image_index NULL: member m is alone
// in image m, which needs M <= N; nothing is written and the arrays may be NULL.
inline ImageGroups image_groups(const int32_t* image_index, int M, int N, int32_t* img_off, int32_t* member_of, int32_t* slot) {
    if (!image_index) return ImageGroups{M > N ? ImageGroups::kNullTooMany : ImageGroups::kOk, 0, 0, 1};
    ImageGroups g;
    for (int m = 0; m < M; ++m)
        if (image_index[m] < 0 || image_index[m] >= N) return ImageGroups{ImageGroups::kOutside, m, image_index[m], 0};
    for (int n = 0; n <= N; ++n) img_off[n] = 0;
    for (int m = 0; m < M; ++m) {
        const int32_t rank = img_off[image_index[m] + 1]++;
        if (slot) slot[m] = rank;
    }
    for (int n = 0; n < N; ++n) {
        if (img_off[n + 1] > g.most) g.most = img_off[n + 1];
        img_off[n + 1] += img_off[n];
    }
    for (int m = 0; m < M; ++m) member_of[img_off[image_index[m]]++] = m;      // img_off[n] is now the end of image n ...
    for (int n = N; n > 0; --n) img_off[n] = img_off[n - 1];                   // ... which is where image n + 1 begins
    img_off[0] = 0;
    return g;
}

}  // namespace gator
