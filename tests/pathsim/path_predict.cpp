// Host build of the predicted path (csrc/cgo_path.hpp: ls_predicted_path) for tests/test_path_predict.py, which compiles this
// file into a small shared library of its own.  Nothing here is a product code path: the product calls the same function from
// Solver::path_points (csrc/cgo_engine.cpp).
#include "cgo_path.hpp"

extern "C" {

// pts[7] ← the steps the line search is predicted to ask for; returns how many (0: not predicted)
int path_predict(const cgo_ls_config *ls, double f, double dphi0, double c, double a_initial, double *pts) {
    double p[7];
    const int k = cgo::ls_predicted_path(*ls, f, dphi0, c, a_initial, p);
    for (int j = 0; j < 7; ++j) pts[j] = p[j];
    return k;
}

// the seven-point tree around a0 (ls_trial_points_n), for comparison
int path_tree(const cgo_ls_config *ls, double a0, double *pts) {
    double p[7];
    const int k = cgo::ls_trial_points_n(*ls, a0, 7, p);
    for (int j = 0; j < 7; ++j) pts[j] = p[j];
    return k;
}

double path_first_step(const cgo_ls_config *ls, double a_initial) { return cgo::ls_first_step(*ls, a_initial); }

}
