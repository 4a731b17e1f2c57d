// host nucleus sampler check: reads 50277 float logits and 50277 float counts from two files, prints nucleus_u() for each u on the command line
// usage: nucleus_app logits.bin counts.bin|- temp top_p top_k presence frequency ban0 u0 [u1 ...]
//        nucleus_app --count counts.bin decay pick0 [pick1 ...]   (applies nucleus_count() per pick, rewrites the file)
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "rwkv_sampler.h"

static bool read_floats(const char *path, std::vector<float> &v)
{
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    const bool ok = fread(v.data(), sizeof(float), v.size(), f) == v.size();
    fclose(f);
    return ok;
}

int main(int argc, char **argv)
{
    std::vector<float> l(50277), c(50277);
    if (argc >= 5 && std::string(argv[1]) == "--count") {
        if (!read_floats(argv[2], c)) return 3;
        for (int i = 4; i < argc; i++) {
            const int g = atoi(argv[i]);
            if (g < 0 || g >= 50277) return 2;
            nucleus_count(c.data(), g, (float)atof(argv[3]));
        }
        FILE *o = fopen(argv[2], "wb");
        if (!o || fwrite(c.data(), sizeof(float), c.size(), o) != c.size()) return 5;
        fclose(o);
        return 0;
    }
    if (argc < 10) return 2;
    if (!read_floats(argv[1], l)) return 3;
    const bool counted = std::string(argv[2]) != "-";
    if (counted && !read_floats(argv[2], c)) return 3;
    const float temp = (float)atof(argv[3]), top_p = (float)atof(argv[4]);
    const unsigned top_k = (unsigned)strtoul(argv[5], nullptr, 10);
    const float presence = (float)atof(argv[6]), frequency = (float)atof(argv[7]);
    const bool ban0 = atoi(argv[8]) != 0;
    const std::vector<double> w = nucleus_weights(l.data(), counted ? c.data() : nullptr, temp, top_p, top_k, presence, frequency, ban0);
    for (int i = 9; i < argc; i++) {
        const int t = nucleus_u(l.data(), counted ? c.data() : nullptr, temp, top_p, top_k, atof(argv[i]), presence, frequency, ban0);
        if (t < 0 || t >= 50277 || !(w[t] > 0)) return 4;      // a pick is a kept token
        printf("%d\n", t);
    }
    return 0;
}
