// cgo_capi_internal.hpp — what the translation units of the extern "C" boundary share (cgo_capi.hip, cgo_capi_batch.hip):
// the handles behind the opaque pointers of include/cgo.h, the guards every entry point is wrapped in, and the two functions of
// cgo_capi.hip the batched entry points call.
#pragma once
#include <string>

#include "cgo_hip_backend.hpp"

// Lifetimes: an objective keeps its context alive and a solver keeps its objective alive, whatever order the host
// destroys the handles in (a garbage-collected host — Python at interpreter exit, Julia finalizers — gives no order).
// cgo_*_destroy drops the HOST's reference; the object goes when the last reference does.
struct cgo_ctx { cgo::HipCtx c; int refs = 1; cgo_solver_policy defpol; bool has_defpol = false; };
struct cgo_objective { cgo::HipObjective o; cgo_ctx *owner = nullptr; int refs = 1; };
inline void ctx_unref(cgo_ctx *c) { if (c && --c->refs == 0) delete c; }
inline void obj_unref(cgo_objective *o) {
    if (o && --o->refs == 0) {
        cgo_ctx *c = o->owner;
        if (c) (void)hipSetDevice(c->c.device);
        delete o;
        ctx_unref(c);
    }
}
struct cgo_solver {
    cgo_ctx *ctx;
    cgo_objective *obj;
    cgo::HipBackend *be;
    cgo::Solver *sv;
    cgo_solver_policy pol;   // what it runs with (cgo_solver_get_policy)
    ~cgo_solver() { delete sv; delete be; if (obj && obj->o.users > 0) obj->o.users--; }
};

#define API_GUARD_BEGIN try {
#define API_GUARD_END                                                        \
    } catch (const std::bad_alloc &) { cgo::set_error("out of host memory"); return CGO_ENOMEM; } \
    catch (const std::exception &e) { cgo::set_error(std::string("internal: ") + e.what()); return CGO_EINVAL; } \
    catch (...) { cgo::set_error("internal: unknown exception"); return CGO_EINVAL; }

#define REQUIRE(cond, msg) do { if (!(cond)) { cgo::set_error(msg); return CGO_EINVAL; } } while (0)
#define HIPCHK2(expr) do { hipError_t e__ = (expr); if (e__ != hipSuccess) { \
    cgo::set_error(std::string("HIP error: ") + hipGetErrorString(e__) + " at " #expr); return CGO_EHIP; } } while (0)

// cgo_capi.hip: explicit argument > context default > CGO_* experiment override > library policy, field by field …
int resolve_policy(cgo_ctx *ctx, const cgo_solver_policy *arg, cgo_solver_policy &r, std::string &why);
// … and the solver of a checked (ctx, objective, config, line search), launch policy decided
int make_solver(cgo_ctx *ctx, cgo_objective *obj, const cgo_cg_config *cfg, const cgo_ls_config *ls,
                const cgo_lss_config *lss, const cgo_solver_policy *policy, cgo_solver **out);
