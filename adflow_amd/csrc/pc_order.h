// Orderings of the ILU(k) over the whole level (adflow_gpu_pc_set_ordering): the reverse Cuthill-McKee ordering of the cell graph and
// the check of a caller's permutation.  Host only: plain C++ without HIP and without globals, so that a stand-alone program can
// include it (tests/host/pc_order_main.cpp).
//
// A permutation is perm[new] = old, 0-based.  The graph is given as CSR: the neighbours of cell c are adj[xadj[c] .. xadj[c + 1] - 1],
// symmetric, without the diagonal, in ascending order.
//
// pc_order_rcm is GENRCM of George and Liu (Computer Solution of Large Sparse Positive Definite Systems, 1981, ch. 4): the connected
// components in the order of their lowest-numbered cell; per component a pseudo-peripheral root, Cuthill-McKee from it, reversed.
// PETSc's MATORDERINGRCM calls SPARSEPACK's routine of that name; identity with the index set PETSc returns is not claimed -- a host
// that wants PETSc's numbers hands over PETSc's own permutation (adflow_gpu_pc_set_ordering_perm).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

// 0: perm[0 .. n-1] is a permutation of 0 .. n-1.  1: perm[*bad] lies outside 0 .. n-1.  2: the value perm[*bad] occurred before.
// *bad is the first offending index.
inline int pc_order_check_perm(const int32_t* perm, long n, long* bad)
{
    std::vector<unsigned char> seen((size_t)(n > 0 ? n : 0), 0);
    for (long a = 0; a < n; ++a) {
        const long c = perm[a];
        if (c < 0 || c >= n) { *bad = a; return 1; }
        if (seen[(size_t)c]) { *bad = a; return 2; }
        seen[(size_t)c] = 1;
    }
    return 0;
}

// the rooted level structure of the component of `root` among the cells with mask != 0: ls = the cells level after level, a cell's
// unvisited neighbours in adjacency order; xls[l] = first cell of level l, and the end.  The mask is restored.
inline void pc_order_rootls(int root, const std::vector<size_t>& xadj, const std::vector<int>& adj, std::vector<unsigned char>& mask,
                            std::vector<int>& ls, std::vector<size_t>& xls)
{
    ls.assign(1, root);
    xls.assign(1, 0);
    mask[(size_t)root] = 0;
    size_t lbegin = 0, lvlend = 1;
    while (lbegin < lvlend) {
        for (size_t i = lbegin; i < lvlend; ++i) {
            const int c = ls[i];
            for (size_t e = xadj[(size_t)c]; e < xadj[(size_t)c + 1]; ++e)
                if (mask[(size_t)adj[e]]) {
                    mask[(size_t)adj[e]] = 0;
                    ls.push_back(adj[e]);
                }
        }
        xls.push_back(lvlend);
        lbegin = lvlend;
        lvlend = ls.size();
    }
    for (int c : ls) mask[(size_t)c] = 1;
}

// perm[new] = old of the reverse Cuthill-McKee ordering of the graph of n cells
inline void pc_order_rcm(long n, const std::vector<size_t>& xadj, const std::vector<int>& adj, std::vector<int>& perm)
{
    perm.clear();
    perm.reserve((size_t)n);
    std::vector<unsigned char> mask((size_t)n, 1);
    std::vector<int> ls, ls2;
    std::vector<size_t> xls, xls2;
    auto deg = [&](int c) { return xadj[(size_t)c + 1] - xadj[(size_t)c]; };       // a component holds every neighbour of its cells
    for (long start = 0; start < n; ++start) {
        if (!mask[(size_t)start]) continue;
        // ---- the pseudo-peripheral root
        int root = (int)start;
        pc_order_rootls(root, xadj, adj, mask, ls, xls);
        const size_t ccsize = ls.size();
        size_t nlvl = xls.size() - 1;
        while (nlvl > 1 && nlvl < ccsize) {
            int cand = ls[xls[nlvl - 1]];
            for (size_t i = xls[nlvl - 1] + 1; i < xls[nlvl]; ++i)
                if (deg(ls[i]) < deg(cand)) cand = ls[i];
            pc_order_rootls(cand, xadj, adj, mask, ls2, xls2);
            root = cand;
            const size_t nun = xls2.size() - 1;
            ls.swap(ls2);
            xls.swap(xls2);
            if (nun <= nlvl) break;
            nlvl = nun;
        }
        // ---- Cuthill-McKee from the root: the newly numbered neighbours of a cell in ascending degree, stable
        const size_t first = perm.size();
        perm.push_back(root);
        mask[(size_t)root] = 0;
        for (size_t at = first; at < perm.size(); ++at) {
            const int c = perm[at];
            const size_t r0 = perm.size();
            for (size_t e = xadj[(size_t)c]; e < xadj[(size_t)c + 1]; ++e)
                if (mask[(size_t)adj[e]]) {
                    mask[(size_t)adj[e]] = 0;
                    perm.push_back(adj[e]);
                }
            std::stable_sort(perm.begin() + (std::ptrdiff_t)r0, perm.end(), [&](int a, int b) { return deg(a) < deg(b); });
        }
        std::reverse(perm.begin() + (std::ptrdiff_t)first, perm.end());
    }
}
