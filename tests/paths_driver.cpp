// Stand-alone driver of juicer_amd/csrc/jd_paths.h (no HIP): a description of jd_debug_paths per line of standard input, a line of output each -
//   refused:  "-1 | <message>"
//   accepted: "0 <out_words> <per stream: the checksums of its images rec, srec, items, dirtyl, tot, item_end, paths, and of the token and item
//             paths read back out of the images> |"
// (checksum: sum of (i + 1) * word i, the words as unsigned, modulo 2^64, printed as a decimal).  tests/test_paths_ref_cpu.py runs it plain and
// under -fsanitize=address,undefined.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "jd_paths.h"

static unsigned long long checksum(const std::vector<int32_t> &w)
{
    unsigned long long h = 0;
    for (size_t i = 0; i < w.size(); ++i) h += (unsigned long long)(uint32_t)w[i] * (unsigned long long)(i + 1);
    return h;
}

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::vector<int32_t> w;
        long long v;
        while (in >> v) w.push_back((int32_t)v);
        PdDesc D;
        std::string err;
        if (!pd_parse(w.data(), (long long)w.size(), &D, &err)) { printf("-1 | %s\n", err.c_str()); continue; }
        printf("0 %lld", D.out_words);
        for (const PdStream &S : D.streams) {
            std::vector<int32_t> rec, img, img2;
            pd_image_rec(D, S, &rec);
            printf(" %llu", checksum(rec));
            pd_image_srec(D, S, &img);
            printf(" %llu", checksum(img));
            std::vector<int32_t> items;
            pd_image_items(D, S, &items);
            printf(" %llu", checksum(items));
            pd_image_dirty(D, S, &img);
            printf(" %llu", checksum(img));
            pd_image_counts(D, S, &img, &img2);
            printf(" %llu %llu", checksum(img), checksum(img2));
            pd_image_paths(S, &img);
            printf(" %llu", checksum(img));
            std::vector<int32_t> back((size_t)(S.n_inst_all * D.NE));
            pd_read_rec(D, S, rec, back.data());
            printf(" %llu", checksum(back));
            back.assign((size_t)S.n_items_all, 0);
            pd_read_items(D, S, items, back.data());
            printf(" %llu", checksum(back));
        }
        printf(" |\n");
    }
    return 0;
}
