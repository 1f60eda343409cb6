/* lcx_coal_floor_probe.h -- one entry point of liblcx_hip.so outside the ABI of include/lcx.h: the floor under the cell maxima of the
 * coalescence bound as the library computes it (lcx_coal_prevote.hpp coal_cmax_floor), on the host, for tools/coal_floor_gate.py.
 * words[0], words[1] = the bits of R_f^2 and V_f as floats for a time step, a cell volume, a scale factor, a largest multiplicity, the
 * efficiency table's end (um) and its running maxima, and a bound eps (<= 0: the production value).  lcx_core.hip includes this header, so
 * a definition that drifts from the declaration does not compile. */
#pragma once
#ifdef __cplusplus
extern "C" {
#endif
void lcx_coal_cmax_floor(double dt, double dvc, double scl, double n_max, double r_max, const double *emax, int n_emax, double eps, unsigned *words);
#ifdef __cplusplus
}
#endif
