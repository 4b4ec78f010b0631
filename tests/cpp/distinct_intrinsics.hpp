// Gives every frame of a generated scene its own fx, fy, u0 and v0 (zero skew, what the resident core takes) and maps the frame's
// observations by the affine map that keeps each the projection of the same ray (tests/hetero_cases.py):
//     u' = f0 (fx' (u k22 / f0 - u0) / fx + u0') / k22     (likewise v)
// srk_scene_generate writes one K into every frame, so an adapter that handed the wrong frame's matrix on would pass without this.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

inline void distinct_intrinsics(int32_t M, double f0, std::vector<double>& K, const std::vector<int32_t>& fr, std::vector<double>& uv)
{
    const std::vector<double> old(K);
    for (int32_t j = 0; j < M; ++j) {
        double* k = &K[9 * (size_t)j];
        const double fx = k[0], fy = k[4];
        k[0] = fx * (1 + 0.15 * std::sin(1.0 + 3.0 * j));
        k[4] = fy * (1 + 0.15 * std::cos(2.0 + 5.0 * j));
        k[2] += 0.15 * fx * std::sin(4.0 + 7.0 * j);
        k[5] += 0.15 * fy * std::cos(3.0 + 11.0 * j);
    }
    for (size_t o = 0; o < fr.size(); ++o) {
        const double *a = &old[9 * (size_t)fr[o]], *b = &K[9 * (size_t)fr[o]];
        uv[2 * o] = f0 * (b[0] * (uv[2 * o] * a[8] / f0 - a[2]) / a[0] + b[2]) / a[8];
        uv[2 * o + 1] = f0 * (b[4] * (uv[2 * o + 1] * a[8] / f0 - a[5]) / a[4] + b[5]) / a[8];
    }
}

// true when no two frames share fx, fy, u0 or v0
inline bool intrinsics_are_distinct(int32_t M, const std::vector<double>& K)
{
    for (int32_t i = 0; i < M; ++i)
        for (int32_t j = i + 1; j < M; ++j)
            for (int e : { 0, 4, 2, 5 })
                if (K[9 * (size_t)i + e] == K[9 * (size_t)j + e]) return false;
    return true;
}
