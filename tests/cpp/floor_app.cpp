// minp_u / mirostat_u for tests/test_floor_cpu.py: floor_app logits.bin counts.bin|- minp|mirostat temp par eta mu0 presence frequency ban0 u...
#include "rwkv_sampler.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

int main(int argc, char **argv)
{
    std::vector<float> v[2];
    for (int k = 0; k < 2 && argc > 11; k++) {
        FILE *f = strcmp(argv[1 + k], "-") ? fopen(argv[1 + k], "rb") : nullptr;
        v[k].resize(f ? 50277 : 0);
        if (f && fread(v[k].data(), 4, 50277, f) != 50277) return 2;
    }
    if (v[0].empty()) return 2;
    const float *c = v[1].empty() ? nullptr : v[1].data();
    const float temp = atof(argv[4]), par = atof(argv[5]), eta = atof(argv[6]), pr = atof(argv[8]), fr = atof(argv[9]), ban0 = atof(argv[10]);
    double mu = atof(argv[7]);
    for (int i = 11; i < argc; i++) {
        const double u = atof(argv[i]);
        const int g = strcmp(argv[3], "minp") ? mirostat_u(v[0].data(), c, temp, par, eta, &mu, u, pr, fr, ban0 != 0) : minp_u(v[0].data(), c, temp, par, u, pr, fr, ban0 != 0);
        printf("%d %.17g\n", g, mu);
    }
    return 0;
}
