// TEST INFRASTRUCTURE -- NOT PRODUCT CODE.  A stand-alone program around adflow_amd/csrc/pc_order.h for tests/test_pc_order_host.py,
// which builds it with the address and undefined-behaviour sanitizers.
//   pc_order_main rcm IN OUT     IN: n, then per cell its degree and its neighbours (ascending); OUT: perm[new] = old, one per line
//   pc_order_main check IN       IN: n, then n values; prints "code index" of pc_order_check_perm
#include <cstdio>
#include <cstring>
#include <vector>

#include "pc_order.h"

int main(int argc, char** argv)
{
    if (argc < 3) return 2;
    FILE* in = fopen(argv[2], "r");
    if (!in) return 2;
    long n = 0;
    if (fscanf(in, "%ld", &n) != 1 || n < 0) return 2;
    if (!strcmp(argv[1], "check")) {
        std::vector<int32_t> p((size_t)n);
        for (long a = 0; a < n; ++a) {
            int v;
            if (fscanf(in, "%d", &v) != 1) return 2;
            p[(size_t)a] = v;
        }
        fclose(in);
        long bad = -1;
        const int rc = pc_order_check_perm(p.data(), n, &bad);
        printf("%d %ld\n", rc, rc ? bad : -1L);
        return 0;
    }
    if (strcmp(argv[1], "rcm") || argc < 4) return 2;
    std::vector<size_t> xadj((size_t)n + 1, 0);
    std::vector<int> adj;
    for (long c = 0; c < n; ++c) {
        int deg;
        if (fscanf(in, "%d", &deg) != 1) return 2;
        for (int e = 0; e < deg; ++e) {
            int m;
            if (fscanf(in, "%d", &m) != 1) return 2;
            adj.push_back(m);
        }
        xadj[(size_t)c + 1] = adj.size();
    }
    fclose(in);
    std::vector<int> perm;
    pc_order_rcm(n, xadj, adj, perm);
    FILE* out = fopen(argv[3], "w");
    if (!out) return 2;
    for (int v : perm) fprintf(out, "%d\n", v);
    fclose(out);
    return 0;
}
