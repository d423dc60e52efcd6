// capi_nd.hip -- the N-D moment filters of the C ABI (include/mfs_hip.h), d = 2 and d = 3: one host path (plan creation, run,
// geometry, destruction, host-pointer entry) over the plan type, and per family what truly differs -- the checks on the model,
// the graded-lex tables, the kernel choice and the switches.  No kernel header is included.
#include <hip/hip_runtime.h>

#include <cstring>
#include <new>

#include "host_run.hpp"

using mfs::fail;

// what the d = 2 and d = 3 plans share: the run's shape, two figures of the plan's kernel and the device copies of the tables
struct NdPlanBase {
    int mode, N, T, B, device;
    int lds_bytes = 0;
    int carry_doubles = 0;      // per replicate, of the block that takes the state across launches; 0: the kernel has none
    double* d_coef = nullptr;
    double* d_lik = nullptr;
    int32_t* d_inds = nullptr;
    double* d_jcoef = nullptr;  // the joint factors' polynomials and parameters (d = 3), or null
    double* d_jpar = nullptr;
};

struct mfs_plan_nd : NdPlanBase {
    static constexpr int kDim = 2;
    static constexpr size_t kPad = 0;
    mfs::FilterNdLaunch launch = nullptr;   // the kernel family of the model, resolved at creation
    mfs::FilterNdArgs args;   // model part filled at create (device pointers), data pointers per run
};

struct mfs_plan_nd3 : NdPlanBase {
    static constexpr int kDim = 3;
    // The host entries lease 8 bytes beyond ys and beyond each [B][T] output.  No kernel reads or writes them (the pool hands
    // out no empty block, which is what they were for at T = 0); they stay so that no block of these entries gets smaller.
    static constexpr size_t kPad = 8;
    // the kernel of the model, resolved at creation: `launch_joint` (with `joint`) if it has joint factors, else `launch`
    mfs::FilterNd3Launch launch = nullptr;
    mfs::FilterNd3JointLaunch launch_joint = nullptr;
    mfs::FilterNd3Args args;  // model part filled at create (device pointers), data pointers per run
    mfs::FilterNd3Joint joint;
};

// what a family's model check tells the shared path about the tables and the kernel
struct NdShape {
    int rows, used_rows;   // coefficient blocks per table, and how many of them the kernel reads
    int S;                 // the index tables are [kDim + 1][S][S]
    int lds_bytes, carry_doubles;
};

// packed true extents of one [D]^d coefficient block (trailing zero rows / columns / planes cut) over ntab tables `stride`
// doubles apart: ea | eb << 8 (| ec << 16 at d = 3); 0: the block is zero everywhere
static int nd_block_extents(const double* blk, int d, size_t D, size_t ntab, size_t stride) {
    int ext[3] = {0, 0, 0};
    size_t n = 1;
    for (int k = 0; k < d; ++k) n *= D;
    for (size_t r = 0; r < ntab; ++r)
        for (size_t q = 0; q < n; ++q)
            if (blk[r * stride + q] != 0.0) {
                size_t rest = q;
                for (int k = d - 1; k >= 0; --k, rest /= D)
                    if ((int)(rest % D) + 1 > ext[k]) ext[k] = (int)(rest % D) + 1;
            }
    return (ext[0] == 0) ? 0 : (ext[0] | (ext[1] << 8) | (ext[2] << 16));
}

// ---------------------------------------------------------------------------------------------------------------
// d = 2: model checks, graded-lex tables, kernel choice and switches
// ---------------------------------------------------------------------------------------------------------------
static int check_nd_model(const mfs_model_nd* model, const void*, int N, int z, NdShape* sh) {
    if (N < 2 || N > mfs::kNdMaxN) return fail(MFS_EUNSUPPORTED, "N = %d outside [2, %d] for d = 2", N, mfs::kNdMaxN);
    const mfs::NdEntry& ke = mfs::g_nd_table[N];
    if (!ke.launch) return fail(MFS_EUNSUPPORTED, "no N-D kernel compiled for N = %d", N);
    if (model->trans_kind != MFS_ND_TRANS_OPERATOR && model->trans_kind != MFS_ND_TRANS_GAUSSIAN)
        return fail(MFS_EINVAL, "unknown N-D transition kind %d", model->trans_kind);
    if (model->trans_kind == MFS_ND_TRANS_GAUSSIAN && model->n_terms != 5)
        return fail(MFS_EINVAL, "the Gaussian N-D transition carries 5 polynomials (mu_0, mu_1, S_00, S_01, S_11)");
    if (model->n_terms < 0 || model->n_terms > MFS_ND_TERMS_MAX) return fail(MFS_EINVAL, "bad n_terms %d", model->n_terms);
    if (z != ke.Z) return fail(MFS_EINVAL, "The size of multi_indices %d must match that of the moments %d.", z, ke.Z);
    const int max_extent = (model->trans_kind == MFS_ND_TRANS_OPERATOR && model->n_terms > MFS_ND_TERMS) ? MFS_ND_MAX_EXTENT_HI : MFS_ND_MAX_EXTENT;
    if (model->extent < 1 || model->extent > max_extent)
        return fail(MFS_EUNSUPPORTED, "coefficient extent %d outside [1, %d]", model->extent, max_extent);
    if (model->n_factors < 1 || model->n_factors > MFS_ND_MAX_FACTORS)
        return fail(MFS_EINVAL, "n_factors %d outside [1, %d]", model->n_factors, MFS_ND_MAX_FACTORS);
    if (model->ny < 1 || model->ny > 2) return fail(MFS_EINVAL, "ny %d outside [1, 2]", model->ny);
    for (int f = 0; f < model->n_factors; ++f) {
        const bool joint = model->fac_kind[f] == MFS_LIK_BEARING_GAUSSIAN;     // a factor of both components: component 2
        if (model->fac_kind[f] < 0 || model->fac_kind[f] > MFS_LIK_BEARING_GAUSSIAN || model->fac_n_par[f] < 1 ||
            model->fac_n_par[f] > MFS_MAX_LIK || model->fac_component[f] < 0 || model->fac_component[f] > 2 ||
            (model->fac_component[f] == 2) != joint || model->fac_ycol[f] < 0 || model->fac_ycol[f] >= model->ny)
            return fail(MFS_EINVAL, "bad description of likelihood factor %d", f);
        if (joint && (model->n_factors != 1 || (model->trans_kind == MFS_ND_TRANS_OPERATOR && (model->n_terms > MFS_ND_TERMS || N > 6))))
            return fail(MFS_EUNSUPPORTED, "a likelihood of both state components: one such factor, with a Normal-closure transition or "
                                          "operator tables of TME order <= 2 at N <= 6 (the other kernels' tiles have no room for the "
                                          "node tables)");
    }
    sh->lds_bytes = ke.lds_bytes; sh->carry_doubles = ke.carry_doubles;
    sh->rows = sh->used_rows = MFS_ND_TABLE_ROWS(model->n_terms);     // 16, or 29 when terms with |kappa| > 4 are present (TME order 3)
    sh->S = ke.S;
    return MFS_OK;
}

static int check_nd_tables(const mfs_model_nd*, int N, int S, int, const int32_t* multi_indices, const int32_t* inds) {
    // The kernels compute the gather of quadratures.py:151-152 arithmetically from the graded-lex order of
    // multi_indices.py:139-229 (d = 2: the index of (a0, a1) is (a0 + a1)(a0 + a1 + 1) / 2 + a0); a caller's table must be that one.
    auto deg = [](int i) { int m = 0; while ((m + 1) * (m + 2) / 2 <= i) ++m; return m; };
    for (int t = 0; t < 3; ++t)
        for (int i = 0; i < S; ++i)
            for (int j = 0; j < S; ++j) {
                const int mi = deg(i), mj = deg(j), ui = i - mi * (mi + 1) / 2, uj = j - mj * (mj + 1) / 2;
                const int M = mi + mj + (t > 0), want = M * (M + 1) / 2 + ui + uj + (t == 1);
                if (inds[(size_t)t * S * S + i * S + j] != want)
                    return fail(MFS_EUNSUPPORTED, "inds[%d][%d][%d] = %d is not the graded-lexicographic Gram / Hankel table (expected %d)",
                                t, i, j, inds[(size_t)t * S * S + i * S + j], want);
            }
    // the kernel derives a moment's multi-index from its position: insist on the graded-lex table
    for (int s = 0, zi = 0; s < 2 * N; ++s)
        for (int n0 = 0; n0 <= s; ++n0, ++zi)
            if (multi_indices[2 * zi] != n0 || multi_indices[2 * zi + 1] != s - n0)
                return fail(MFS_EINVAL, "multi_indices is not the graded-lexicographic table of order 2N-1");
    return MFS_OK;
}

static hipError_t finish_nd_plan(mfs_plan_nd* p, const mfs_model_nd* model, const void*, int stable) {
    const mfs::NdEntry& ke = mfs::g_nd_table[p->N];
    // the kernel family: Normal closure; operator table with |kappa| > 4 terms (TME order 3: the 29-row layout); operator
    // table with the node tables of a joint likelihood; operator table
    const bool joint = model->n_factors == 1 && model->fac_component[0] == 2;
    p->launch = (model->trans_kind == MFS_ND_TRANS_GAUSSIAN) ? ke.launch_gauss
                : (model->n_terms > MFS_ND_TERMS) ? ke.launch_hi : joint ? ke.launch_joint : ke.launch;
    mfs::FilterNdArgs& a = p->args;
    a.stable = stable; a.n_terms_used = model->n_terms;
    // stable = 1: the completion on the register front end (a.stable = 1); MFS_ND_STABLE=dense keeps the LDS-tile form (2)
    if (stable) { const char* e = getenv("MFS_ND_STABLE"); a.stable = (e && strcmp(e, "dense") == 0) ? 2 : 1; }
    if (const char* e = getenv("MFS_ND_UPDATE")) {   // A/B switches, like MFS_SOLVER
        a.force_eigen = (strcmp(e, "eigen") == 0);
        a.joint_grid = (strcmp(e, "grid") == 0);
    }
    return hipSuccess;
}

static int create_failed(const mfs_plan_nd*, hipError_t e) {
    return fail(e == hipErrorOutOfMemory ? MFS_ENOMEM : MFS_EHIP, "mfs_plan_nd_create: %s", hipGetErrorString(e));
}

// one launch over the steps [t0, t1) of the plan's run; `carry` ([B][carry_doubles], or null for a single launch over [0, T))
// takes the state from one chunk to the next
static int nd_launch(mfs_plan_nd* p, const mfs::FilterRun& run, int t0, int t1, double* carry, hipStream_t stream) {
    mfs::FilterNdArgs a = p->args;
    mfs::set_run(a, p->mode, run);
    a.t_begin = t0; a.t_end = t1; a.carry = carry;
    const hipError_t e = p->launch(a, p->B, stream);
    if (e != hipSuccess) return fail(MFS_EHIP, "N-D kernel launch: %s", hipGetErrorString(e));
    return MFS_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// d = 3: the same.  joint == nullptr: the model of mfs_plan_nd3_create (1..3 single-component factors, ny <= 3)
// ---------------------------------------------------------------------------------------------------------------
static int check_nd_model(const mfs_model_nd3* model, const mfs_joint_nd3* joint, int N, int z, NdShape* sh) {
    if (N < MFS_ND3_MIN_N || N > MFS_ND3_MAX_N)
        return fail(MFS_EUNSUPPORTED, "N = %d outside [%d, %d] for d = 3", N, MFS_ND3_MIN_N, MFS_ND3_MAX_N);
    const mfs::Nd3Entry& ke = mfs::g_nd3_table[N];
    if (!ke.launch) return fail(MFS_EUNSUPPORTED, "no d = 3 kernel compiled for N = %d", N);
    if (model->trans_kind != MFS_ND_TRANS_OPERATOR && model->trans_kind != MFS_ND_TRANS_GAUSSIAN)
        return fail(MFS_EINVAL, "unknown N-D transition kind %d", model->trans_kind);
    const bool gauss = model->trans_kind == MFS_ND_TRANS_GAUSSIAN;
    if (model->n_terms != (gauss ? MFS_ND3_GAUSS_TERMS : MFS_ND3_TERMS))
        return fail(MFS_EINVAL, "n_terms %d: the d = 3 tables carry %d operator terms or %d Normal-closure polynomials",
                    model->n_terms, MFS_ND3_TERMS, MFS_ND3_GAUSS_TERMS);
    if (z != ke.Z) return fail(MFS_EINVAL, "The size of multi_indices %d must match that of the moments %d.", z, ke.Z);
    if (model->extent < 1 || model->extent > MFS_ND3_MAX_EXTENT)
        return fail(MFS_EUNSUPPORTED, "coefficient extent %d outside [1, %d]", model->extent, MFS_ND3_MAX_EXTENT);
    const int min_factors = joint ? 0 : 1, max_ny = joint ? MFS_ND3_JOINT_MAX_NY : 3;
    if (model->n_factors < min_factors || model->n_factors > MFS_ND3_MAX_FACTORS)
        return fail(MFS_EINVAL, "n_factors %d outside [%d, %d]", model->n_factors, min_factors, MFS_ND3_MAX_FACTORS);
    if (model->ny < 1 || model->ny > max_ny) return fail(MFS_EINVAL, "ny %d outside [1, %d]", model->ny, max_ny);
    if (joint) {
        if (joint->n_joint < 1 || joint->n_joint > MFS_ND3_MAX_JOINT)
            return fail(MFS_EINVAL, "n_joint %d outside [1, %d]", joint->n_joint, MFS_ND3_MAX_JOINT);
        if (joint->extent < 1 || joint->extent > MFS_ND3_JOINT_MAX_EXTENT)
            return fail(MFS_EUNSUPPORTED, "joint polynomial extent %d outside [1, %d]", joint->extent, MFS_ND3_JOINT_MAX_EXTENT);
        for (int f = 0; f < joint->n_joint; ++f) {
            if (joint->kind[f] < 0 || joint->kind[f] > MFS_LIK_GAUSSIAN)
                return fail(MFS_EINVAL, "joint factor %d: kind %d is not Bernoulli-logistic, Poisson-softplus or Gaussian", f, joint->kind[f]);
            if (joint->link[f] < MFS_ND3_LINK_POLY || joint->link[f] > MFS_ND3_LINK_ATAN2_SQRT)
                return fail(MFS_EINVAL, "joint factor %d: unknown link %d", f, joint->link[f]);
            if (joint->ycol[f] < 0 || joint->ycol[f] >= model->ny)
                return fail(MFS_EINVAL, "joint factor %d: measurement column %d outside [0, ny = %d)", f, joint->ycol[f], model->ny);
        }
        if (!joint->coef || !joint->par) return fail(MFS_EINVAL, "NULL buffer");
    }
    for (int f = 0; f < model->n_factors; ++f) {
        if (model->fac_kind[f] == MFS_LIK_BEARING_GAUSSIAN)
            return fail(MFS_EUNSUPPORTED, "a likelihood of several state components is not supported at d = 3");
        if (model->fac_kind[f] < 0 || model->fac_kind[f] > MFS_LIK_GAUSSIAN || model->fac_n_par[f] < 1 ||
            model->fac_n_par[f] > MFS_MAX_LIK || model->fac_component[f] < 0 || model->fac_component[f] > 2 ||
            model->fac_ycol[f] < 0 || model->fac_ycol[f] >= model->ny)
            return fail(MFS_EINVAL, "bad description of likelihood factor %d", f);
    }
    sh->lds_bytes = ke.lds_bytes; sh->carry_doubles = 0;      // (no carry block: a run is one launch)
    sh->rows = MFS_ND3_ROWS; sh->used_rows = gauss ? MFS_ND3_GAUSS_TERMS : MFS_ND3_ROWS;
    sh->S = ke.S;
    return MFS_OK;
}

static int check_nd_tables(const mfs_model_nd3*, int, int S, int z, const int32_t* multi_indices, const int32_t* inds) {
    // the kernel derives a moment's multi-index from its position: insist on the graded-lex tables
    for (int zi = 0; zi < z; ++zi)
        for (int k = 0; k < 3; ++k)
            if (multi_indices[3 * zi + k] != mfs::nd3_exp(zi, k))
                return fail(MFS_EINVAL, "multi_indices is not the graded-lexicographic table of order 2N-1");
    for (int t = 0; t < 4; ++t)
        for (int i = 0; i < S; ++i)
            for (int j = 0; j < S; ++j) {
                const int want = mfs::nd3_index(mfs::nd3_exp(i, 0) + mfs::nd3_exp(j, 0) + (t == 1),
                                                mfs::nd3_exp(i, 1) + mfs::nd3_exp(j, 1) + (t == 2),
                                                mfs::nd3_exp(i, 2) + mfs::nd3_exp(j, 2) + (t == 3));
                if (inds[((size_t)t * S + i) * S + j] != want)
                    return fail(MFS_EUNSUPPORTED, "inds[%d][%d][%d] = %d is not the graded-lexicographic Gram / Hankel table (expected %d)",
                                t, i, j, inds[((size_t)t * S + i) * S + j], want);
            }
    return MFS_OK;
}

static hipError_t finish_nd_plan(mfs_plan_nd3* p, const mfs_model_nd3* model, const mfs_joint_nd3* joint, int stable) {
    const mfs::Nd3Entry& ke = mfs::g_nd3_table[p->N];
    const bool gauss = model->trans_kind == MFS_ND_TRANS_GAUSSIAN;
    if (joint) p->launch_joint = gauss ? ke.joint_gauss : ke.joint;
    else p->launch = gauss ? ke.launch_gauss : ke.launch;
    p->args.stable = stable ? 1 : 0; p->args.trans_kind = model->trans_kind;
    mfs::FilterNd3Joint& jt = p->joint;
    memset(&jt, 0, sizeof(jt));
    if (!joint) return hipSuccess;
    const size_t E = (size_t)joint->extent, jblk = 2 * E * E * E, jtab = (size_t)joint->n_joint * jblk;
    const size_t njb = joint->batched ? (size_t)p->B : 1, njpar = njb * joint->n_joint;
    mfs::BlockPool<false>& pool = mfs::device_state(p->device).device;
    hipError_t e = pool.acquire((void**)&p->d_jcoef, njb * jtab * 8);
    if (e == hipSuccess) e = pool.acquire((void**)&p->d_jpar, njpar * 8);
    if (e == hipSuccess && njb) e = hipMemcpy(p->d_jcoef, joint->coef, njb * jtab * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess && njb) e = hipMemcpy(p->d_jpar, joint->par, njpar * 8, hipMemcpyHostToDevice);
    jt.n = joint->n_joint; jt.E = joint->extent; jt.batched = joint->batched ? 1 : 0;
    for (int f = 0; f < joint->n_joint; ++f) {
        jt.kind[f] = joint->kind[f]; jt.link[f] = joint->link[f]; jt.ycol[f] = joint->ycol[f];
        for (int w = 0; w < 2; ++w)
            jt.ext[f][w] = nd_block_extents(joint->coef + (size_t)f * jblk + (size_t)w * E * E * E, 3, E, njb, jtab);
    }
    jt.coef = p->d_jcoef; jt.par = p->d_jpar;
    return e;
}

static int create_failed(const mfs_plan_nd3*, hipError_t e) {
    return fail(e == hipErrorOutOfMemory ? MFS_ENOMEM : MFS_EHIP, "mfs_plan_nd3_create: %s", hipGetErrorString(e));
}

// the whole run in one launch (the kernel takes no step range and no carry)
static int nd_launch(mfs_plan_nd3* p, const mfs::FilterRun& run, int, int, double*, hipStream_t stream) {
    mfs::FilterNd3Args a = p->args;
    mfs::set_run(a, p->mode, run);
    const hipError_t e = p->launch_joint ? p->launch_joint(a, p->joint, p->B, stream) : p->launch(a, p->B, stream);
    if (e != hipSuccess) return fail(MFS_EHIP, "d = 3 kernel launch: %s", hipGetErrorString(e));
    return MFS_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// the host path of both
// ---------------------------------------------------------------------------------------------------------------
template <typename Plan>
static void destroy_nd_plan(Plan* p, bool quiesced) {
    hipSetDevice(p->device);
    if (!quiesced) hipDeviceSynchronize();   // pool blocks must be idle when they go back (what hipFree did implicitly)
    mfs::BlockPool<false>& pool = mfs::device_state(p->device).device;
    for (void* b : {(void*)p->d_coef, (void*)p->d_lik, (void*)p->d_inds, (void*)p->d_jcoef, (void*)p->d_jpar}) pool.release(b);
    delete p;
}

// Joint: mfs_joint_nd3 at d = 3; d = 2 has no such description and passes a null void pointer
template <typename Plan, typename Model, typename Joint>
static int nd_plan_create(Plan** plan, const Model* model, const Joint* joint, int mode, int N, int T, int B, int z,
                          const int32_t* multi_indices, const int32_t* inds, int stable, int device) {
    if (!plan) return fail(MFS_EINVAL, "plan is NULL");
    *plan = nullptr;
    if (!model) return fail(MFS_EINVAL, "model is NULL");
    if (mode != MFS_MODE_RAW && mode != MFS_MODE_CENTRAL && mode != MFS_MODE_SCALED)
        return fail(MFS_EINVAL, "unknown moment mode %d", mode);
    NdShape sh;
    if (int rc = check_nd_model(model, joint, N, z, &sh)) return rc;
    if (T < 0 || B < 0) return fail(MFS_EINVAL, "negative T or B");
    if (!multi_indices || !inds || !model->coef || (model->n_factors > 0 && !model->lik)) return fail(MFS_EINVAL, "NULL buffer");
    if (int rc = check_nd_tables(model, N, sh.S, z, multi_indices, inds)) return rc;
    HIP_TRY(hipSetDevice(device));
    Plan* p = new (std::nothrow) Plan();
    if (!p) return fail(MFS_ENOMEM, "out of host memory");
    p->mode = mode; p->N = N; p->T = T; p->B = B; p->device = device;
    p->lds_bytes = sh.lds_bytes; p->carry_doubles = sh.carry_doubles;

    // pool blocks for the coefficient, likelihood-parameter and Gram / Hankel index tables, and their upload
    size_t block = 1;
    for (int k = 0; k < Plan::kDim; ++k) block *= (size_t)model->extent;
    const size_t ntab = model->coef_batched ? (size_t)B : 1, ncoef = ntab * sh.rows * block;
    const size_t nlik = (size_t)(model->lik_batched ? B : 1) * model->n_factors * MFS_MAX_LIK;
    const size_t ninds = (size_t)(Plan::kDim + 1) * sh.S * sh.S;
    mfs::BlockPool<false>& pool = mfs::device_state(device).device;
    hipError_t e = pool.acquire((void**)&p->d_coef, ncoef * 8);
    if (e == hipSuccess) e = pool.acquire((void**)&p->d_lik, nlik * 8);
    if (e == hipSuccess) e = pool.acquire((void**)&p->d_inds, ninds * 4);
    if (e == hipSuccess && ncoef) e = hipMemcpy(p->d_coef, model->coef, ncoef * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess && nlik) e = hipMemcpy(p->d_lik, model->lik, nlik * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(p->d_inds, inds, ninds * 4, hipMemcpyHostToDevice);

    // the part of the kernel arguments that both model structs describe alike, then the family's own
    auto& a = p->args;
    memset(&a, 0, sizeof(a));
    a.mode = mode; a.T = T; a.B = B;
    a.D = model->extent; a.n_factors = model->n_factors; a.ny = model->ny;
    for (int f = 0; f < model->n_factors; ++f) {
        a.fac_kind[f] = model->fac_kind[f]; a.fac_comp[f] = model->fac_component[f]; a.fac_ycol[f] = model->fac_ycol[f];
    }
    a.coef_batched = model->coef_batched; a.lik_batched = model->lik_batched;
    a.coef = p->d_coef; a.lik = p->d_lik; a.inds = p->d_inds;
    // true extents of each coefficient block the kernel reads; the union over replicates when batched
    for (int k = 0; k < sh.used_rows; ++k)
        a.ext[k] = nd_block_extents(model->coef + (size_t)k * block, Plan::kDim, (size_t)model->extent, ntab, sh.rows * block);
    if (e == hipSuccess) e = finish_nd_plan(p, model, joint, stable);
    if (e != hipSuccess) {
        destroy_nd_plan(p, true);
        return create_failed((const Plan*)nullptr, e);
    }
    *plan = p;
    return MFS_OK;
}

template <typename Plan>
static int nd_plan_run(Plan* p, const mfs::FilterRun& run, void* stream) {
    if (!p) return fail(MFS_EINVAL, "plan is NULL");
    // (an empty batch returns before its pointers are looked at, unlike mfs_plan_1d_run: the codes these entries have always given)
    if (p->B == 0) return MFS_OK;
    if (int rc = mfs::check_run_pointers(p->mode, run.m0, run.mean0, run.scale0, run.ys, run.out_nell, p->T, p->B)) return rc;
    HIP_TRY(hipSetDevice(p->device));
    return nd_launch(p, run, 0, p->T, nullptr, (hipStream_t)stream);
}

static int nd_plan_geometry(const NdPlanBase* p, int* threads_per_filter, int* grid, int* lds_bytes_per_block) {
    if (!p) return fail(MFS_EINVAL, "plan is NULL");
    if (threads_per_filter) *threads_per_filter = 256;
    if (grid) *grid = p->B;
    if (lds_bytes_per_block) *lds_bytes_per_block = p->lds_bytes;
    return MFS_OK;
}

// The host-pointer entry on a plan made for it, which it destroys.  With the moments streamed out in chunks, the per-replicate
// state crosses the launches through a carry block, so the bits are those of the single launch; a kernel without a carry
// block (d = 3) runs in one launch, its moments copied after it.
template <typename Plan>
static int nd_filter(const char* name, Plan* plan, int ny, int z, const double* m0, int m0_batched, const double* mean0,
                     const double* scale0, const double* ys, double* out_moments, double* out_means, double* out_scales,
                     double* out_nell, int32_t* out_first_nan, void* stream) {
    struct Guard { Plan* p; ~Guard() { destroy_nd_plan(p, true); } } guard{plan};   // (every exit below is quiesced)
    const int mode = plan->mode, T = plan->T, B = plan->B, device = plan->device;
    if (int rc = mfs::check_run_pointers(mode, m0, mean0, scale0, ys, out_nell, T, B)) return rc;
    if (B == 0) return MFS_OK;
    mfs::Staging st(device, stream, true);
    const mfs::FilterRun run = mfs::stage_filter_run(st, mode, B, T, m0_batched ? B : 1, (size_t)z, Plan::kDim, (size_t)ny, Plan::kPad,
                                                     m0, m0_batched, mean0, scale0, ys, out_moments, out_means, out_scales,
                                                     out_nell, out_first_nan);
    const int nchunks = plan->carry_doubles ? mfs::host_chunks(device, T, B, (size_t)z, out_moments != nullptr) : 1;
    double* d_carry = (nchunks > 1) ? st.work((size_t)B * plan->carry_doubles * 8) : nullptr;
    const int rc = mfs::run_streaming_out(st, T, B, nchunks, (size_t)z, out_moments, run.out_mom, [&](int t0, int t1) {
        return nd_launch(plan, run, t0, t1, d_carry, st.s);
    });
    if (rc == MFS_OK) st.download();
    return st.finish(name, rc);
}

extern "C" {

int mfs_plan_nd_create(mfs_plan_nd** plan, const mfs_model_nd* model, int mode, int N, int T, int B, int z,
                       const int32_t* multi_indices, const int32_t* inds, int stable, int device) {
    // (asked before the mode, as it always was)
    if (plan && model && model->d != 2) {
        *plan = nullptr;
        return fail(MFS_EUNSUPPORTED, "the device N-D path supports d = 2 (got %d)", model->d);
    }
    return nd_plan_create(plan, model, (const void*)nullptr, mode, N, T, B, z, multi_indices, inds, stable, device);
}

int mfs_plan_nd3_create(mfs_plan_nd3** plan, const mfs_model_nd3* model, int mode, int N, int T, int B, int z,
                        const int32_t* multi_indices, const int32_t* inds, int stable, int device) {
    return nd_plan_create(plan, model, (const mfs_joint_nd3*)nullptr, mode, N, T, B, z, multi_indices, inds, stable, device);
}

int mfs_plan_nd3_create_joint(mfs_plan_nd3** plan, const mfs_model_nd3* model, const mfs_joint_nd3* joint, int mode, int N, int T,
                              int B, int z, const int32_t* multi_indices, const int32_t* inds, int stable, int device) {
    if (plan) *plan = nullptr;
    if (!joint) return fail(MFS_EINVAL, "joint is NULL (a model without joint factors goes through mfs_plan_nd3_create)");
    return nd_plan_create(plan, model, joint, mode, N, T, B, z, multi_indices, inds, stable, device);
}

int mfs_plan_nd_run(mfs_plan_nd* p, const double* d_m0, int m0_batched, const double* d_mean0, const double* d_scale0,
                    const double* d_ys, double* d_out_moments, double* d_out_means, double* d_out_scales, double* d_out_nell,
                    int32_t* d_out_first_nan, void* stream) {
    return nd_plan_run(p, mfs::FilterRun{d_m0, m0_batched, d_mean0, d_scale0, d_ys, d_out_moments, d_out_means, d_out_scales,
                                         d_out_nell, d_out_first_nan}, stream);
}

int mfs_plan_nd3_run(mfs_plan_nd3* p, const double* d_m0, int m0_batched, const double* d_mean0, const double* d_scale0,
                     const double* d_ys, double* d_out_moments, double* d_out_means, double* d_out_scales, double* d_out_nell,
                     int32_t* d_out_first_nan, void* stream) {
    return nd_plan_run(p, mfs::FilterRun{d_m0, m0_batched, d_mean0, d_scale0, d_ys, d_out_moments, d_out_means, d_out_scales,
                                         d_out_nell, d_out_first_nan}, stream);
}

int mfs_plan_nd_destroy(mfs_plan_nd* p) {
    if (p) destroy_nd_plan(p, false);
    return MFS_OK;
}

int mfs_plan_nd3_destroy(mfs_plan_nd3* p) {
    if (p) destroy_nd_plan(p, false);
    return MFS_OK;
}

int mfs_plan_nd_geometry(const mfs_plan_nd* p, int* threads_per_filter, int* grid, int* lds_bytes_per_block) {
    return nd_plan_geometry(p, threads_per_filter, grid, lds_bytes_per_block);
}

int mfs_plan_nd3_geometry(const mfs_plan_nd3* p, int* threads_per_filter, int* grid, int* lds_bytes_per_block) {
    return nd_plan_geometry(p, threads_per_filter, grid, lds_bytes_per_block);
}

int mfs_filter_nd(const mfs_model_nd* model, int mode, int N, int T, int B, int z, const int32_t* multi_indices,
                  const int32_t* inds, const double* m0, int m0_batched, const double* mean0, const double* scale0,
                  const double* ys, int stable, double* out_moments, double* out_means, double* out_scales, double* out_nell,
                  int32_t* out_first_nan, int device, void* stream) {
    mfs_plan_nd* plan = nullptr;
    if (int rc = mfs_plan_nd_create(&plan, model, mode, N, T, B, z, multi_indices, inds, stable, device)) return rc;
    return nd_filter("mfs_filter_nd", plan, model->ny, z, m0, m0_batched, mean0, scale0, ys, out_moments, out_means, out_scales,
                     out_nell, out_first_nan, stream);
}

int mfs_filter_nd3(const mfs_model_nd3* model, int mode, int N, int T, int B, int z, const int32_t* multi_indices,
                   const int32_t* inds, const double* m0, int m0_batched, const double* mean0, const double* scale0,
                   const double* ys, int stable, double* out_moments, double* out_means, double* out_scales, double* out_nell,
                   int32_t* out_first_nan, int device, void* stream) {
    mfs_plan_nd3* plan = nullptr;
    if (int rc = mfs_plan_nd3_create(&plan, model, mode, N, T, B, z, multi_indices, inds, stable, device)) return rc;
    return nd_filter("mfs_filter_nd3", plan, model->ny, z, m0, m0_batched, mean0, scale0, ys, out_moments, out_means, out_scales,
                     out_nell, out_first_nan, stream);
}

int mfs_filter_nd3_joint(const mfs_model_nd3* model, const mfs_joint_nd3* joint, int mode, int N, int T, int B, int z,
                         const int32_t* multi_indices, const int32_t* inds, const double* m0, int m0_batched, const double* mean0,
                         const double* scale0, const double* ys, int stable, double* out_moments, double* out_means,
                         double* out_scales, double* out_nell, int32_t* out_first_nan, int device, void* stream) {
    if (!joint) return fail(MFS_EINVAL, "joint is NULL (a model without joint factors goes through mfs_filter_nd3)");
    mfs_plan_nd3* plan = nullptr;
    if (int rc = mfs_plan_nd3_create_joint(&plan, model, joint, mode, N, T, B, z, multi_indices, inds, stable, device)) return rc;
    return nd_filter("mfs_filter_nd3", plan, model->ny, z, m0, m0_batched, mean0, scale0, ys, out_moments, out_means, out_scales,
                     out_nell, out_first_nan, stream);
}

}  // extern "C"
