// bsx_adam_step.hip -- the optimiser step between bsx_actor_grad and the next bsx_actor_forward (include/battlespace_hip.h: bsx_adam_step*), gfx950.
//
// torch's clip_grad_norm_ + Adam.step() over one or two StackedActor networks (and the Gaussian head's log_std), from the [A, G] gradient
// rows bsx_actor_grad writes to the updated parameters, the Adam moments and the packed weight blobs bsx_actor_forward reads -- the
// parameters are ~5 000 floats per agent, so the whole step is two launches:
//   1. norm  -- one workgroup per (network, agent) row (one more for log_std): the float64 sum of squares of the row's real elements (the
//               pad columns of w3 / b3 are skipped), per thread over a fixed stride, then a shuffle tree, then the waves in order -> one
//               partial per workgroup.  Workgroup 0 also reads `step` and `hyper`, stores step + 1 and leaves the call's scalars -- the
//               two bias corrections formed in float64 -- in the workspace.
//   2. apply -- one workgroup per row again.  Every workgroup adds the (at most 65) partials in the same fixed order, so all of them
//               hold the same norm and clip coefficient without a third launch; updates its row's moments and parameters (float32), keeps
//               the new parameters in LDS in the row's layout and writes every float of the row's blob from there.  Workgroup 0 writes stats.
// `step` and `hyper` are read on the device at every launch: a captured graph follows a learning-rate schedule and counts its own steps.
// No floating-point atomics, no flags or spins; the grid is a function of (n, nets, log_std given) alone: the same inputs give the same bits.
//
// bsx_adam_step_shared ties the agents in consecutive groups of `group` to one set of parameters: the gradient of a shared parameter is
// the float32 sum of its members' rows in agent order.  The same two launches over the same grid: every member's workgroup forms the
// group's sum for itself, in both passes -- no workgroup writes another's row, nothing is added to the workspace -- and only a leader's
// workgroup (the first agent of a group) contributes a partial norm, so a shared parameter counts once.  group = 1 is bsx_adam_step:
// the sum is the row's own element.  Both kernels are templates on TIED: the untied call's instances hold no loop over members.
//
// bsx_adam_step_mlp is the one path behind all three entries: any (A, D) the fused MLP kernels take (A <= 32, odd allowed, D <= 64: a row
// of up to 8 836 floats, 35 KB of LDS), any group that divides A, and per network an optional Polyak target.  A workgroup whose network
// has a target goes on after its blob: t = (1 - tau) t + tau p per element against its own LDS image of the new parameters, the blended
// value back into the image, and the target's blob from the image by the same blob_float -- no second image, no further launch.  tau is
// hyper[5], read in the apply pass.  The Polyak work is the template parameter POLYAK of the apply body: the instances without it
// (bsx_adam_apply_kernel, every call in which no network has a target) hold no load or branch for it and take the kernel argument
// they always took: the targets' pointers ride in the Polyak instances' argument alone.

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "battlespace_hip.h"
#include "bsx_actor_layout.h"
#include "bsx_args.h"
#include "bsx_block_sum.h"

namespace {

using namespace bsx_actor;

constexpr int NORM_TPB = 1024;                            // a row is 5 .. 9 floats per thread: the passes are latency, not bandwidth
constexpr int APPLY_TPB = 1024;
constexpr int D_MAX = BSX_MLP_MAX_D;
constexpr int G_MAX = grad_floats(D_MAX);
constexpr int SCALARS = 8;                                // workspace doubles ahead of the partials: t | lr | lr / (1 - b1^t) | sqrt(1 - b2^t) | b1 | b2 | eps | max_norm
constexpr int PART_MAX = 4 * BSX_MAX_N + 1;
static_assert(G_MAX == 8836 && G_MAX * sizeof(float) + 64 <= 64 * 1024, "the apply pass keeps one row in static LDS");

struct Args {
    BsxAdamIo io;
    int A, D, rows, parts;                                // rows = nets * A network rows; parts = rows (+ 1 with log_std)
    double* ws;
    double* stats;
    int group;                                            // agents per tied group, consecutive; 1 = every agent on its own (last: the untied instances never load it)
};
// the argument of the Polyak instances alone: a call without targets passes the 176 bytes of pointers to no kernel
struct PolyakArgs {
    Args a;
    BsxAdamTargets tg;                                    // all NULL for a network without a target
};

// where element j of a gradient row lives: k = the parameter's index in learner.PARAMS, i = the float inside agent a's slice of it;
// false = a pad column of w3 / b3 (no parameter behind it)
struct Where { int k, i; };
__device__ inline bool locate(int j, int D, int na, Where& w) {
    if (j < row_b1(D)) { w.k = 0; w.i = j; return true; }
    if (j < row_w2(D)) { const int r = j - row_b1(D); w.k = 1 + r / H; w.i = r % H; return true; }
    if (j < row_b2(D)) { w.k = 4; w.i = j - row_w2(D); return true; }
    if (j < row_w3(D)) { const int r = j - row_b2(D); w.k = 5 + r / H; w.i = r % H; return true; }
    if (j < row_b3(D)) { const int r = j - row_w3(D), c = r & 3; w.k = 8; w.i = (r >> 2) * na + c; return c < na; }
    const int c = j - row_b3(D);
    w.k = 9; w.i = c;
    return c < na;
}

__device__ inline int param_row_floats(int k, int D, int na) {
    return k == 0 ? H * D : k == 4 ? H * H : k == 8 ? H * na : k == 9 ? na : H;
}

// the network of a workgroup, field by field with constant indices: a dynamic index into the by-value argument, or a copy of the
// struct with its pointer array, would go through private memory
struct Net { const float* grad; float* m; float* v; float* blob; int na; };
__device__ inline Net pick(const BsxAdamIo& io, int net) {
    const bool second = net == 1;
    Net N;
    N.grad = second ? io.net[1].grad : io.net[0].grad;
    N.m = second ? io.net[1].m : io.net[0].m;
    N.v = second ? io.net[1].v : io.net[0].v;
    N.blob = second ? io.net[1].blob : io.net[0].blob;
    N.na = second ? io.net[1].n_actions : io.net[0].n_actions;
    return N;
}

__device__ inline float* param_ptr(const BsxAdamIo& io, int net, int k) {
    const bool second = net == 1;
    float* p = second ? io.net[1].p[0] : io.net[0].p[0];
#pragma unroll
    for (int q = 1; q < 10; ++q) p = k == q ? (second ? io.net[1].p[q] : io.net[0].p[q]) : p;
    return p;
}

// parameter k of one network's target, with constant indices like param_ptr
__device__ inline float* target_ptr(const BsxAdamTarget& T, int k) {
    float* p = T.p[0];
#pragma unroll
    for (int q = 1; q < 10; ++q) p = k == q ? T.p[q] : p;
    return p;
}

// element j of a group's gradient: its `group` members' rows (`stride` floats apart, the leader's first) added in agent order, plain
// float32 additions from the leader's value on -- ((g_l + g_l+1) + g_l+2) + ...; untied (group = 1) the leader's own element
template <int TIED>
__device__ inline float group_grad(const float* leader, int j, int stride, int group) {
    float s = leader[j];
    if constexpr (TIED) {
#pragma unroll 4
        for (int k = 1; k < group; ++k) s += leader[size_t(k) * stride + j];
    }
    return s;
}

template <int TIED>
__global__ __launch_bounds__(NORM_TPB) void bsx_adam_norm_kernel(const Args p) {
    __shared__ double s_w[NORM_TPB / 64];
    const int tid = threadIdx.x, b = blockIdx.x;
    double acc = 0.0;
    if (b < p.rows) {
        const int net = b / p.A, a = b - net * p.A;
        const Net N = pick(p.io, net);
        const int G = grad_floats(p.D);
        const float* g = N.grad + size_t(a) * G;
        if constexpr (!TIED) {
#pragma unroll 4
            for (int j = tid; j < G; j += NORM_TPB) {
                Where w;
                const double x = double(g[j]);
                if (locate(j, p.D, N.na, w)) acc += x * x;
            }
        } else if (a % p.group == 0) {                           // a leader: the group's sum counts once; a follower's partial is +0
            for (int j = tid; j < G; j += NORM_TPB) {
                Where w;
                if (locate(j, p.D, N.na, w)) { const double x = double(group_grad<1>(g, j, G, p.group)); acc += x * x; }
            }
        }
    } else {
        for (int j = tid; j < 3 * p.A; j += NORM_TPB) {
            if (TIED && (j / 3) % p.group) continue;             // leader rows only
            const double x = double(group_grad<TIED>(p.io.g_log_std, j, 3, p.group));
            acc += x * x;
        }
    }
    acc = block_sum<double, NORM_TPB / 64>(acc, s_w);
    if (tid == 0) {
        p.ws[SCALARS + b] = acc;
        if (b == 0) {
            const int64_t t = *p.io.step + 1;
            *p.io.step = t;
            const double lr = double(p.io.hyper[0]), b1 = double(p.io.hyper[1]), b2 = double(p.io.hyper[2]);
            p.ws[0] = double(t);
            p.ws[1] = lr;
            p.ws[2] = lr / (1.0 - pow(b1, double(t)));
            p.ws[3] = sqrt(1.0 - pow(b2, double(t)));
            p.ws[4] = b1;
            p.ws[5] = b2;
            p.ws[6] = double(p.io.hyper[3]);
            p.ws[7] = double(p.io.hyper[4]);
        }
    }
}

__device__ inline uint32_t bf16_rne(float x) {                  // torch's float32 -> bfloat16: round to nearest even, a NaN to the quiet NaN
    const uint32_t u = __float_as_uint(x);
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0u;
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}
__device__ inline float bf16_float(uint32_t h) { return __uint_as_float(h << 16); }

// term 0 / 1 / 2 of W2B's split of w, residuals in float32 as StackedActor.pack() takes them
__device__ inline uint32_t w2b_term(float w, int term) {
    const uint32_t h = bf16_rne(w);
    if (term == 0) return h;
    const float r1 = w - bf16_float(h);
    const uint32_t m = bf16_rne(r1);
    if (term == 1) return m;
    return bf16_rne(r1 - bf16_float(m));
}

// float f of an agent's blob from its parameters in the gradient row's layout (s: LDS, pad columns of w3 / b3 hold +0)
__device__ inline float blob_float(const float* s, int f, int D) {
    const int Dp = dpad(D);
    if (f < off_w2(D)) {                                         // W1A[mo][s][lane]
        const int lane = f & 63, r = f >> 6, hp = Dp / 2, mo = r / hp, sp = r - mo * hp;
        const int k = 2 * sp + (lane >> 5), j = 32 * mo + (lane & 31);
        return k < D ? s[k * H + j] : 0.0f;                      // (w1 is the head of the row)
    }
    if (f < off_small(D)) {                                      // W2A[mo][mt][vq][lane][t]
        const int r = f - off_w2(D);
        return s[row_w2(D) + w2a_k(r) * H + w2a_j(r)];
    }
    if (f < off_w3(D)) {                                         // b1 g1 h1 b2 g2 h2, each [hh][mo][v]
        const int r = f - off_small(D);
        const int vec = r >> 6, q = r & 63, v = q & 15, mo = (q >> 4) & 1, hh = q >> 5;
        return s[(vec < 3 ? row_b1(D) + vec * H : row_b2(D) + (vec - 3) * H) + nid(mo, v, hh)];
    }
    if (f < off_b3(D)) {                                         // W3P[hh][mt][v][4]
        const int r = f - off_w3(D);
        const int c = r & 3, v = (r >> 2) & 15, mt = (r >> 6) & 1, hh = r >> 7;
        return s[row_w3(D) + nid(mt, v, hh) * NA + c];
    }
    if (f < off_w2b(D)) return s[row_b3(D) + (f - off_b3(D))];
    // W2B[mo][s][term][lane][i], two bfloat16 (i even, i + 1) per float slot, the even one in the low half
    const int e = 2 * (f - off_w2b(D));
    const int i = e & 7, lane = (e >> 3) & 63, rest = e >> 9, term = rest % 3, sq = (rest / 3) & 3, mo = rest / 12;
    const int col = 32 * mo + (lane & 31), hh = lane >> 5;
    const float w0 = s[row_w2(D) + nid(sq >> 1, 8 * (sq & 1) + i, hh) * H + col];
    const float w1 = s[row_w2(D) + nid(sq >> 1, 8 * (sq & 1) + i + 1, hh) * H + col];
    return __uint_as_float(w2b_term(w0, term) | (w2b_term(w1, term) << 16));
}

struct Scalars { float coef, b1, omb1, b2, omb2, step_size, bc2_sqrt, eps; };

// one element of Adam: g = coef grad; m = b1 m + (1 - b1) g; v = b2 v + (1 - b2) g^2; p -= step_size m / (sqrt(v) / sqrt(1 - b2^t) + eps)
__device__ inline float adam_element(const Scalars& c, float grad, float& m, float& v, float p) {
    const float g = c.coef * grad;
    m = c.b1 * m + c.omb1 * g;
    v = c.b2 * v + c.omb2 * (g * g);
    const float denom = sqrtf(v) / c.bc2_sqrt + c.eps;
    return p - c.step_size * (m / denom);
}

// the Polyak half of a workgroup whose network has target T (T.blob = nullptr: it has none): t = (1 - tau) t + tau p per element
// against the LDS image s of the new parameters, the blended value back into the image, the target's blob row from the image
__device__ __forceinline__ void polyak_row(const BsxAdamTarget& T, float tau, float* s, int a, int D, int na) {
    if (!T.blob) return;                                         // (the whole workgroup: no barrier is left behind)
    const int tid = threadIdx.x, G = grad_floats(D), BF = blob_floats(D);
    float* tblob = T.blob + size_t(a) * BF;
    const float omt = float(1.0 - double(tau));
    __syncthreads();                                             // the blob pass has read the image
    for (int j = tid; j < G; j += APPLY_TPB) {                   // thread and j as in the first loop: the pad columns keep their +0
        Where w;
        if (locate(j, D, na, w)) {
            float* q = target_ptr(T, w.k) + size_t(a) * param_row_floats(w.k, D, na) + w.i;
            const float t = fmaf(omt, *q, tau * s[j]);
            *q = t;
            s[j] = t;
        }
    }
    __syncthreads();
    for (int f = tid; f < BF; f += APPLY_TPB) tblob[f] = blob_float(s, f, D);
}

template <int TIED, int POLYAK>
__device__ __forceinline__ void apply_body(const Args& p, const BsxAdamTargets* tg) {
    __shared__ float s_p[G_MAX];
    __shared__ double s_norm2;
    const int tid = threadIdx.x, b = blockIdx.x;
    if (tid < 64) {                                              // the partials, two per lane at most, by the same tree in every workgroup
        double x = tid < p.parts ? p.ws[SCALARS + tid] : 0.0;
        if (tid + 64 < p.parts) x += p.ws[SCALARS + tid + 64];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
        if (tid == 0) s_norm2 = x;
    }
    __syncthreads();
    const double norm = sqrt(s_norm2), max_norm = p.ws[7];
    double coef = 1.0;
    if (max_norm > 0.0) {
        const double q = max_norm / (norm + 1e-6);
        coef = q < 1.0 ? q : 1.0;
    }
    Scalars c;
    c.coef = float(coef);
    c.b1 = float(p.ws[4]); c.omb1 = float(1.0 - p.ws[4]);
    c.b2 = float(p.ws[5]); c.omb2 = float(1.0 - p.ws[5]);
    c.step_size = float(p.ws[2]); c.bc2_sqrt = float(p.ws[3]); c.eps = float(p.ws[6]);
    if (b == 0 && tid == 0) {
        p.stats[0] = p.ws[0];
        p.stats[1] = norm;
        p.stats[2] = coef;
        p.stats[3] = p.ws[1];
    }
    if (b >= p.rows) {                                           // log_std: [A][3], no blob
        for (int j = tid; j < 3 * p.A; j += APPLY_TPB) {
            float m = p.io.m_ls[j], v = p.io.v_ls[j];
            float g;
            if constexpr (TIED) g = group_grad<1>(p.io.g_log_std + 3 * (j / 3 / p.group * p.group), j % 3, 3, p.group);   // from the leader's row on
            else g = p.io.g_log_std[j];
            const float x = adam_element(c, g, m, v, p.io.log_std[j]);
            p.io.m_ls[j] = m; p.io.v_ls[j] = v; p.io.log_std[j] = x;
        }
        return;
    }
    const int net = b / p.A, a = b - net * p.A, D = p.D;
    const Net N = pick(p.io, net);
    const int na = N.na, G = grad_floats(D);
    const float* grad = N.grad + size_t(TIED ? a / p.group * p.group : a) * G;   // tied: the group leader's row
    float* mrow = N.m + size_t(a) * G;
    float* vrow = N.v + size_t(a) * G;
#pragma unroll 2
    for (int j = tid; j < G; j += APPLY_TPB) {
        Where w;
        float x = 0.0f;
        if (locate(j, D, na, w)) {
            float* q = param_ptr(p.io, net, w.k) + size_t(a) * param_row_floats(w.k, D, na) + w.i;
            float m = mrow[j], v = vrow[j];
            x = adam_element(c, group_grad<TIED>(grad, j, G, p.group), m, v, *q);
            mrow[j] = m; vrow[j] = v; *q = x;
        }
        s_p[j] = x;
    }
    __syncthreads();
    const int BF = blob_floats(D);
    float* blob = N.blob + size_t(a) * BF;
    for (int f = tid; f < BF; f += APPLY_TPB) blob[f] = blob_float(s_p, f, D);
    if constexpr (POLYAK) {                                      // (a branch per network, not a select per pointer: eleven pointers live, not twenty-two)
        if (net == 1) polyak_row(tg->net[1], p.io.hyper[5], s_p, a, D, na);
        else polyak_row(tg->net[0], p.io.hyper[5], s_p, a, D, na);
    }
}

template <int TIED>
__global__ __launch_bounds__(APPLY_TPB) void bsx_adam_apply_kernel(const Args p) { apply_body<TIED, 0>(p, nullptr); }

template <int TIED>
__global__ __launch_bounds__(APPLY_TPB) void bsx_adam_apply_polyak_kernel(const PolyakArgs p) { apply_body<TIED, 1>(p.a, &p.tg); }

int check_net(const BsxAdamNet& N) {
    for (int k = 0; k < 10; ++k)
        if (!N.p[k]) return BSX_E_ARG;
    if (!N.grad || !N.m || !N.v || !N.blob) return BSX_E_ARG;
    if (N.n_actions != 1 && N.n_actions != 3 && N.n_actions != 4) return BSX_E_ARG;
    return 0;
}

// 0: no target, 1: a whole one, BSX_E_ARG: some but not all of the eleven pointers
int check_target(const BsxAdamTarget& T) {
    int given = T.blob != nullptr;
    for (int k = 0; k < 10; ++k) given += T.p[k] != nullptr;
    return given == 0 ? 0 : given == 11 ? 1 : BSX_E_ARG;
}

int check_net_align(const BsxAdamNet& N) {
    for (int k = 0; k < 10; ++k)
        if (!aligned(N.p[k], 4)) return BSX_E_ALIGN;
    if (!aligned(N.grad, 16) || !aligned(N.m, 16) || !aligned(N.v, 16) || !aligned(N.blob, 16)) return BSX_E_ALIGN;
    return 0;
}

}  // namespace

extern "C" {

int bsx_adam_step_mlp_workspace_bytes(int A, int nets, size_t* bytes) {
    if (!bytes || A < 1 || A > 2 * BSX_MAX_N || (nets != 1 && nets != 2)) return BSX_E_ARG;
    *bytes = size_t(8) * size_t(SCALARS + nets * A + 1);
    return 0;
}

int bsx_adam_step_workspace_bytes(int n, int nets, size_t* bytes) {
    if (n < 1 || n > BSX_MAX_N) return BSX_E_ARG;
    return bsx_adam_step_mlp_workspace_bytes(2 * n, nets, bytes);
}

int bsx_adam_step(const BsxAdamIo* io, int n, void* workspace, double* stats, void* stream) {
    return bsx_adam_step_shared(io, n, 1, workspace, stats, stream);
}

// the two entries of the actor's shape: their own rules for n and group (BSX_E_ARG, like everything ahead of the alignment rules), then
// the one path at (2n, 3n + 2) without targets
int bsx_adam_step_shared(const BsxAdamIo* io, int n, int group, void* workspace, double* stats, void* stream) {
    if (n < 1 || n > BSX_MAX_N) return BSX_E_ARG;
    if (group != 1 && group != 2 * n && (group < 2 || n % group)) return BSX_E_ARG;
    return bsx_adam_step_mlp(io, 2 * n, 3 * n + 2, group, nullptr, workspace, stats, stream);
}

int bsx_adam_step_mlp(const BsxAdamIo* io, int A, int D, int group, const BsxAdamTargets* targets, void* workspace, double* stats,
                      void* stream) {
    if (!io || !workspace || !stats || !io->hyper || !io->step) return BSX_E_ARG;
    if (A < 1 || A > 2 * BSX_MAX_N || D < 1 || D > BSX_MLP_MAX_D || (io->nets != 1 && io->nets != 2)) return BSX_E_ARG;
    if (group < 1 || A % group) return BSX_E_ARG;
    for (int k = 0; k < io->nets; ++k)
        if (const int rc = check_net(io->net[k])) return rc;
    const int given = (io->log_std != nullptr) + (io->g_log_std != nullptr) + (io->m_ls != nullptr) + (io->v_ls != nullptr);
    if (given != 0 && given != 4) return BSX_E_ARG;
    bool polyak = false;
    for (int k = 0; targets && k < io->nets; ++k) {
        const int rc = check_target(targets->net[k]);
        if (rc < 0) return rc;
        polyak |= rc == 1;
    }
    for (int k = 0; k < io->nets; ++k)
        if (const int rc = check_net_align(io->net[k])) return rc;
    if (!aligned(io->log_std, 4) || !aligned(io->g_log_std, 4) || !aligned(io->m_ls, 4) || !aligned(io->v_ls, 4)) return BSX_E_ALIGN;
    if (!aligned(io->hyper, 4) || !aligned(io->step, 8) || !aligned(workspace, 8) || !aligned(stats, 8)) return BSX_E_ALIGN;
    PolyakArgs pa;
    Args& a = pa.a;
    a.io = *io;
    if (io->nets == 1) a.io.net[1] = io->net[0];                 // never selected; keeps the argument free of unset pointers
    pa.tg = BsxAdamTargets{};
    for (int k = 0; polyak && k < io->nets; ++k) {
        for (int q = 0; q < 10; ++q)
            if (!aligned(targets->net[k].p[q], 4)) return BSX_E_ALIGN;
        if (!aligned(targets->net[k].blob, 16)) return BSX_E_ALIGN;
        pa.tg.net[k] = targets->net[k];
    }
    a.A = A;
    a.D = D;
    a.rows = io->nets * a.A;
    a.parts = a.rows + (given ? 1 : 0);
    a.group = group;
    a.ws = static_cast<double*>(workspace);
    a.stats = stats;
    static_assert(PART_MAX <= 128, "the apply pass adds two partials per lane of one wave");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool tied = group > 1;
    hipLaunchKernelGGL(tied ? bsx_adam_norm_kernel<1> : bsx_adam_norm_kernel<0>, dim3(unsigned(a.parts)), dim3(NORM_TPB), 0, s, a);
    if (const hipError_t e = hipGetLastError()) return int(e);
    if (polyak) hipLaunchKernelGGL(tied ? bsx_adam_apply_polyak_kernel<1> : bsx_adam_apply_polyak_kernel<0>, dim3(unsigned(a.parts)), dim3(APPLY_TPB), 0, s, pa);
    else hipLaunchKernelGGL(tied ? bsx_adam_apply_kernel<1> : bsx_adam_apply_kernel<0>, dim3(unsigned(a.parts)), dim3(APPLY_TPB), 0, s, a);
    return int(hipGetLastError());
}

}  // extern "C"
