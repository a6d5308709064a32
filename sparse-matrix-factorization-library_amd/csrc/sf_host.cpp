// The flat host ABI both struct libraries and the Python layer stand on: sf_version, the sf_symbolic_* accessors, the subtree and
// out-of-core partitions and the orderings, over sf_symbolic.cpp.  No struct header: the struct entry points are in sf_chol_host.cpp
// and sf_lu_host.cpp, and this file links beside either.
#include <sparseframe_flat.h>

#include <new>
#include <string>
#include <vector>

#include "sf_symbolic.h"

using sf::Long;

struct sf_symbolic {
    sf::Symbolic S;
};

extern "C" {

const char* sf_version(void) { return "sparseframe-hip 0.1 (gfx950)"; }

// ------------------------------------------------------------------------------------------
// flat symbolic ABI
// ------------------------------------------------------------------------------------------
int sf_symbolic_create(sf_symbolic** out, sf_long n, const sf_long* Cp, const sf_long* Ci, const sf_float* Cx,
                       const sf_long* perm, size_t devSlotSize) {
    if (!out) return SF_ERR_ARG;
    *out = nullptr;
    sf_symbolic* h = new (std::nothrow) sf_symbolic();
    if (!h) return SF_ERR_ALLOC;
    int rc = sf::analyze_cholesky(n, Cp, Ci, Cx, perm, devSlotSize, h->S);
    if (rc) { delete h; return SF_ERR_ARG; }
    *out = h;
    return SF_OK;
}

int sf_symbolic_create_lu(sf_symbolic** out, sf_long n, const sf_long* Cp, const sf_long* Ci, const sf_float* Cx,
                          const sf_long* perm, size_t devSlotSize, int is_symmetric) {
    if (!out) return SF_ERR_ARG;
    *out = nullptr;
    sf_symbolic* h = new (std::nothrow) sf_symbolic();
    if (!h) return SF_ERR_ALLOC;
    int rc = sf::analyze_lu(n, Cp, Ci, Cx, perm, devSlotSize, is_symmetric != 0, h->S);
    if (rc) { delete h; return SF_ERR_ARG; }
    *out = h;
    return SF_OK;
}

void sf_symbolic_destroy(sf_symbolic* sym) { delete sym; }

sf_long sf_symbolic_scalar(const sf_symbolic* sym, const char* name) {
    if (!sym || !name) return -1;
    const sf::Symbolic& S = sym->S;
    const std::string k(name);
    if (k == "n") return S.n;
    if (k == "nnz") return S.Lp.empty() ? 0 : S.Lp[S.n];
    if (k == "nfsuper") return S.nfsuper;
    if (k == "nsuper") return S.nsuper;
    if (k == "nstage") return S.nstage;
    if (k == "isize") return S.isize;
    if (k == "xsize") return S.xsize;
    if (k == "csize") return S.csize;
    if (k == "nsleaf") return S.nsleaf;
    if (k == "lu") return S.lu ? 1 : 0;
    if (k == "symmetric") return S.symmetric ? 1 : 0;
    if (k == "unz") return S.Up.empty() ? 0 : S.Up[S.n];
    return -1;
}

const sf_long* sf_symbolic_long_array(const sf_symbolic* sym, const char* name, sf_long* len) {
    if (len) *len = 0;
    if (!sym || !name) return nullptr;
    const sf::Symbolic& S = sym->S;
    const std::string k(name);
    const std::vector<Long>* v = nullptr;
    const sf::RawVec<Long>* w = (k == "Li") ? &S.Li : (k == "LTi") ? &S.LTi : (k == "Ui") ? &S.Ui : (k == "UTi") ? &S.UTi : (k == "Lsi") ? &S.Lsi : nullptr;
    if (w) {
        if (len) *len = (sf_long)w->size();
        return (const sf_long*)w->data();
    }
    if (k == "Perm") v = &S.Perm;
    else if (k == "Parent") v = &S.Parent;
    else if (k == "Parent0") v = &S.Parent0;
    else if (k == "Post") v = &S.Post;
    else if (k == "ColCount") v = &S.ColCount;
    else if (k == "ColCount0") v = &S.ColCount0;
    else if (k == "Lp") v = &S.Lp;
    else if (k == "LTp") v = &S.LTp;
    else if (k == "Up") v = &S.Up;
    else if (k == "UTp") v = &S.UTp;
    else if (k == "Super") v = &S.Super;
    else if (k == "SuperMap") v = &S.SuperMap;
    else if (k == "Sparent") v = &S.Sparent;
    else if (k == "Lsip") v = &S.Lsip;
    else if (k == "Lsxp") v = &S.Lsxp;
    else if (k == "LeafQueue") v = &S.LeafQueue;
    else if (k == "ST_Map") v = &S.ST_Map;
    else if (k == "ST_Pointer") v = &S.ST_Pointer;
    else if (k == "ST_Index") v = &S.ST_Index;
    else if (k == "Aoffset") v = &S.Aoffset;
    else if (k == "Moffset") v = &S.Moffset;
    if (!v) return nullptr;
    if (len) *len = (sf_long)v->size();
    return (const sf_long*)v->data();
}

const sf_float* sf_symbolic_float_array(const sf_symbolic* sym, const char* name, sf_long* len) {
    if (len) *len = 0;
    if (!sym || !name) return nullptr;
    const std::string k(name);
    const sf::RawVec<double>* v = nullptr;
    if (k == "Lx") v = &sym->S.Lx;
    else if (k == "LTx") v = &sym->S.LTx;
    else if (k == "Ux") v = &sym->S.Ux;
    else if (k == "UTx") v = &sym->S.UTx;
    if (!v) return nullptr;
    if (len) *len = (sf_long)v->size();
    return v->data();
}

double sf_symbolic_flops(const sf_symbolic* sym, int which) {
    if (!sym) return 0;
    if (which == 0) return sf::flops_struct(sym->S);
    double upd = 0, sc = 0;
    const double all = sf::flops_exec(sym->S, &upd, &sc);
    if (which == 1) return all;
    if (which == 2) return upd;
    if (which == 3) return sc;
    return 0;
}

int sf_subtree_partition(sf_long nsuper, const sf_long* Super, const sf_long* SuperMap, const sf_long* Lsip,
                         const sf_long* Lsi, int nranks, int32_t* owner, double* top_fraction, double* max_load_fraction) {
    if (!Super || !Lsip || (nsuper > 0 && (!SuperMap || !Lsi))) return SF_ERR_ARG;
    return sf::subtree_partition(nsuper, Super, SuperMap, Lsip, Lsi, nranks, owner, top_fraction, max_load_fraction) ? SF_ERR_ARG : SF_OK;
}

int sf_subtree_partition_weighted(sf_long nsuper, const sf_long* Super, const sf_long* SuperMap, const sf_long* Lsip,
                                  const sf_long* Lsi, int nranks, double top_weight, int32_t* owner, double* top_fraction,
                                  double* max_load_fraction) {
    if (!Super || !Lsip || (nsuper > 0 && (!SuperMap || !Lsi))) return SF_ERR_ARG;
    return sf::subtree_partition(nsuper, Super, SuperMap, Lsip, Lsi, nranks, owner, top_fraction, max_load_fraction, top_weight) ? SF_ERR_ARG : SF_OK;
}

int sf_ooc_partition(sf_long nsuper, const sf_long* Super, const sf_long* SuperMap, const sf_long* Lsip, const sf_long* Lsi,
                     sf_long budget_entries, int32_t* group, int* ngroups, sf_long* group_entries, sf_long* top_entries, sf_long* need_entries,
                     int* top_mode) {
    if (!Super || !Lsip || !group || !ngroups || (nsuper > 0 && (!SuperMap || !Lsi))) return SF_ERR_ARG;
    int64_t ge = 0, te = 0, nd = 0;
    int mode = 0;
    const int rc = sf::ooc_partition(nsuper, Super, SuperMap, Lsip, Lsi, budget_entries, group, ngroups, &ge, &te, &nd, &mode);
    if (group_entries) *group_entries = ge;
    if (top_entries) *top_entries = te;
    if (need_entries) *need_entries = nd;
    if (top_mode) *top_mode = mode;
    return rc == 0 ? SF_OK : (rc == 2 ? SF_ERR_ALLOC : SF_ERR_ARG);
}

int sf_graph_nd_perm(sf_long n, const sf_long* Cp, const sf_long* Ci, sf_long leaf, sf_long* perm) {
    return sf::graph_nd_perm(n, Cp, Ci, leaf, perm) ? SF_ERR_ARG : SF_OK;
}

int sf_grid_nd_perm(sf_long nx, sf_long ny, sf_long nz, sf_long leaf, sf_long sep_width, sf_long* perm) {
    return sf::grid_nd_perm(nx, ny, nz, leaf, sep_width, perm) ? SF_ERR_ARG : SF_OK;
}
}  // extern "C"
