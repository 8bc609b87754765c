// ORACLE — TEST INFRASTRUCTURE ONLY (see grid.hpp header).
//
// oracle_capi.cpp: extern "C" entry points so tests/ (ctypes + numpy) can drive the CPU
// restatement.  Arrays are Fortran-order, component outermost (amrex::Array4 layout), FP64.
#include <cstring>
#ifdef _OPENMP
#include <omp.h>
#endif
#include <memory>

#include "amr.hpp"
#include "cooling.hpp"
#include "hydro_sim.hpp"
#include "problems.hpp"

using namespace oracle;

extern "C" {

struct orc_hydro_traits {
	double gamma;
	double cs_isothermal;
	double mean_molecular_weight;
	double boltzmann_constant;
	int reconstruct_eint;
	int nscalars;
	int ndim;
};

static auto makeSystem(orc_hydro_traits const *t) -> HydroSystem
{
	HydroSystem h;
	h.tr.eos.tr.gamma = t->gamma;
	h.tr.eos.tr.cs_isothermal = t->cs_isothermal;
	h.tr.eos.tr.mean_molecular_weight = t->mean_molecular_weight;
	h.tr.eos.tr.boltzmann_constant = t->boltzmann_constant;
	h.tr.reconstruct_eint = (t->reconstruct_eint != 0);
	h.tr.nscalars = t->nscalars;
	h.tr.ndim = t->ndim;
	return h;
}

static auto mkbox(int const lo[3], int const hi[3]) -> Box
{
	Box b;
	for (int d = 0; d < 3; ++d) {
		b.lo[d] = lo[d];
		b.hi[d] = hi[d];
	}
	return b;
}

int orc_eos_variant() { return kEosVariant; }

// ------------------------------------------------------------------ per-operator entry points
// `cons`/`prim` live on `gbox` = valid box grown by nghost (in the first ndim dims).

void orc_cons_to_prim(orc_hydro_traits const *t, double const *cons, double *prim, int const glo[3], int const ghi[3])
{
	HydroSystem h = makeSystem(t);
	Box g = mkbox(glo, ghi);
	h.ConservedToPrimitive(Array4<const double>(cons, g, h.tr.nvar()), Array4<double>(prim, g, h.tr.nvar()), g);
}

void orc_flattening_coefficients(orc_hydro_traits const *t, int dir, double const *prim, int const glo[3], int const ghi[3], double *chi,
				 int const clo[3], int const chi_hi[3])
{
	g_spacedim = t->ndim;
	HydroSystem h = makeSystem(t);
	Box g = mkbox(glo, ghi);
	Box c = mkbox(clo, chi_hi);
	h.ComputeFlatteningCoefficients(dir, Array4<const double>(prim, g, h.tr.nvar()), Array4<double>(chi, c, 1), c);
}

// Full flux evaluation for one box exactly as computeHydroFluxes / computeFOHydroFluxes do it.
// order: 1/2/3 -> donor/PLM-minmod/PPM with flattening + HLLC ; order = 0 -> first-order LLF path
// (computeFOHydroFluxes).  flux_d: face box (nodal in d) x nvar ; fvel_d: face box x 1.
void orc_compute_hydro_fluxes(orc_hydro_traits const *t, int order, double K_visc, double const *cons, int const vlo[3], int const vhi[3], int nghost,
			      double *flux0, double *flux1, double *flux2, double *fvel0, double *fvel1, double *fvel2)
{
	g_spacedim = t->ndim;
	HydroSim sim;
	sim.hydro = makeSystem(t);
	sim.geom.ndim = t->ndim;
	sim.grids = {mkbox(vlo, vhi)};
	sim.nghost_cc = nghost;
	sim.ncomp_cc = sim.hydro.tr.nvar();
	sim.artificialViscosityK_ = K_visc;
	sim.reconstructionOrder_ = (order == 0) ? 1 : (order % 10);
	sim.is_mhd_enabled = (order >= 10); // order + 10: the fluxes of an MHD problem (HLLD with the reference's B = 0 stub)
	order = order % 10;
	int const nv = sim.hydro.tr.nvar();
	MultiFab consMF(sim.grids, nv, nghost, t->ndim);
	std::memcpy(consMF.fabs[0].d.data(), cons, consMF.fabs[0].d.size() * sizeof(double));
	auto result = (order == 0) ? sim.computeFOHydroFluxes(consMF, nv) : sim.computeHydroFluxes(consMF, nv);
	double *fo[3] = {flux0, flux1, flux2};
	double *vo[3] = {fvel0, fvel1, fvel2};
	for (int d = 0; d < t->ndim; ++d) {
		std::memcpy(fo[d], result.first[d].fabs[0].d.data(), result.first[d].fabs[0].d.size() * sizeof(double));
		std::memcpy(vo[d], result.second[d].fabs[0].d.data(), result.second[d].fabs[0].d.size() * sizeof(double));
	}
}

// ------------------------------------------------------------------ the hydro operators on arrays the caller owns (tests/test_hydro_cells_*.py)
// Thin wrappers: boxes and layouts as orc_cons_to_prim.  `v` is the valid box, `g` the box the cell-centred state arrays live on.

// ComputeFluxes<RIEMANN, DIR> (hydro_system.hpp:852-1112) on left / right states and primitives the caller supplies: L, R, flux (nvar components)
// and fvel (one) live on the face box of v in direction dir, prim on v grown by nghost_prim >= 1 in the first ndim directions (it only supplies
// the velocity differences du, dvl, dvr, dwl, dwr).  Every face is an independent sample.
void orc_hydro_face_fluxes(orc_hydro_traits const *t, int riemann, int dir, double K_visc, double const *L, double const *R, double const *prim,
			   int const vlo[3], int const vhi[3], int nghost_prim, double *flux, double *fvel)
{
	g_spacedim = t->ndim;
	HydroSystem const h = makeSystem(t);
	Box const v = mkbox(vlo, vhi);
	Box const f = faceBox(v, dir);
	Box const g = grow(v, nghost_prim, t->ndim);
	int const nv = h.tr.nvar();
	h.ComputeFluxes(riemann, dir, Array4<double>(flux, f, nv), Array4<double>(fvel, f, 1), Array4<const double>(L, f, nv), Array4<const double>(R, f, nv),
			Array4<const double>(prim, g, nv), K_visc, f);
}

// EnforceLimits (hydro_system.hpp:696-773) on the cells of v; the first nmscalars passive scalars are partial densities
void orc_hydro_enforce_limits(orc_hydro_traits const *t, int nmscalars, double densityFloor, double tempFloor, double *state, int const glo[3], int const ghi[3],
			      int const vlo[3], int const vhi[3])
{
	HydroSystem h = makeSystem(t);
	h.tr.nmscalars = nmscalars;
	h.EnforceLimits(densityFloor, tempFloor, Array4<double>(state, mkbox(glo, ghi), h.tr.nvar()), mkbox(vlo, vhi));
}

// SyncDualEnergy (hydro_system.hpp:816-850) on the cells of v.  A cell with rho <= 0 is fatal in the reference (amrex::Abort): here it is left
// untouched and fatal (on v, one int per cell) is set for it; returns the number of such cells.
long orc_hydro_sync_dual_energy(orc_hydro_traits const *t, double *state, int const glo[3], int const ghi[3], int const vlo[3], int const vhi[3], int *fatal)
{
	HydroSystem const h = makeSystem(t);
	Box const v = mkbox(vlo, vhi);
	Array4<double> const U(state, mkbox(glo, ghi), h.tr.nvar());
	Array4<int> const bad(fatal, v, 1);
	long count = 0;
	for (int k = v.lo[2]; k <= v.hi[2]; ++k) {
		for (int j = v.lo[1]; j <= v.hi[1]; ++j) {
			for (int i = v.lo[0]; i <= v.hi[0]; ++i) {
				if (U(i, j, k, density_index) <= 0.) {
					bad(i, j, k) = 1;
					++count;
					continue;
				}
				bad(i, j, k) = 0;
				Box one;
				one.lo[0] = one.hi[0] = i;
				one.lo[1] = one.hi[1] = j;
				one.lo[2] = one.hi[2] = k;
				h.SyncDualEnergy(U, one);
			}
		}
	}
	return count;
}

// ComputeMaxSignalSpeed (hydro_system.hpp:223-252): maxSignal on v, one component
void orc_hydro_max_signal_speed(orc_hydro_traits const *t, double const *cons, int const glo[3], int const ghi[3], int const vlo[3], int const vhi[3],
				double *maxSignal)
{
	HydroSystem const h = makeSystem(t);
	Box const v = mkbox(vlo, vhi);
	h.ComputeMaxSignalSpeed(Array4<const double>(cons, mkbox(glo, ghi), h.tr.nvar()), Array4<double>(maxSignal, v, 1), v);
}

// the serial reduction over v.  which = 0: maxSignalSpeedLocal (hydro_system.hpp:198-221); which = 1: the maximum of ComputeMaxSignalSpeed,
// reduced the same way (result = std::max(result, value) from -infinity: a NaN value never replaces the result).
double orc_hydro_max_signal_local(orc_hydro_traits const *t, int which, double const *cons, int const glo[3], int const ghi[3], int const vlo[3],
				  int const vhi[3])
{
	HydroSystem const h = makeSystem(t);
	Box const v = mkbox(vlo, vhi);
	Array4<const double> const U(cons, mkbox(glo, ghi), h.tr.nvar());
	if (which == 0) {
		return h.maxSignalSpeedLocal(U, v);
	}
	Fab<double> sig(v, 1);
	h.ComputeMaxSignalSpeed(U, sig.array(), v);
	double result = -std::numeric_limits<double>::infinity();
	for (double const s : sig.d) {
		result = std::max(result, s);
	}
	return result;
}

// PredictStep (hydro_system.hpp:475-497) with isStateValid (:423-446): consOld / consNew on g (ncomp components), rhs (nvars components) and
// redoFlag on v; returns the number of flagged cells.  The reference always passes nvars = nvar_; with fewer the scalars of consNew are not this
// call's product and the mass-scalar part of isStateValid does not apply (the rule of qk_hydro_PredictStep, include/quokka_amd.h).
long orc_hydro_predict_step(orc_hydro_traits const *t, int nmscalars, double const *consOld, double *consNew, int ncomp, double const *rhs, double dt, int nvars,
			    int const glo[3], int const ghi[3], int const vlo[3], int const vhi[3], int *redoFlag)
{
	HydroSystem h = makeSystem(t);
	h.tr.nmscalars = (nvars >= kNumHydroVars + nmscalars) ? nmscalars : 0;
	Box const v = mkbox(vlo, vhi);
	Box const g = mkbox(glo, ghi);
	h.PredictStep(Array4<const double>(consOld, g, ncomp), Array4<double>(consNew, g, ncomp), Array4<const double>(rhs, v, nvars), dt, nvars,
		      Array4<int>(redoFlag, v, 1), v);
	long count = 0;
	for (int64_t n = 0; n < v.numPts(); ++n) {
		count += (redoFlag[n] != redo_none) ? 1 : 0;
	}
	return count;
}

// ComputeRhsFromFluxes (hydro_system.hpp:448-473): rhs on v, flux[d] on the face box of v in direction d, nvars components each
void orc_hydro_rhs_from_fluxes(orc_hydro_traits const *t, double *rhs, double const *const flux[3], double const dx[3], int nvars, int const vlo[3],
			       int const vhi[3])
{
	HydroSystem const h = makeSystem(t);
	Box const v = mkbox(vlo, vhi);
	std::array<Array4<const double>, 3> f{};
	for (int d = 0; d < t->ndim; ++d) {
		f[d] = Array4<const double>(flux[d], faceBox(v, d), nvars);
	}
	h.ComputeRhsFromFluxes(Array4<double>(rhs, v, nvars), f, dx, nvars, v);
}

// AddInternalEnergyPdV (hydro_system.hpp:775-814): rhs (ncomp_rhs components) and redoFlag on v, cons on g (>= 1 ghost cell: a flagged cell reads
// its neighbours' velocities), vel[d] on the face box of v in direction d
void orc_hydro_add_pdv(orc_hydro_traits const *t, double *rhs, int ncomp_rhs, double const *cons, int const glo[3], int const ghi[3], double const dx[3],
		       double const *const vel[3], int const *redoFlag, int const vlo[3], int const vhi[3])
{
	HydroSystem const h = makeSystem(t);
	Box const v = mkbox(vlo, vhi);
	std::array<Array4<const double>, 3> f{};
	for (int d = 0; d < t->ndim; ++d) {
		f[d] = Array4<const double>(vel[d], faceBox(v, d), 1);
	}
	h.AddInternalEnergyPdV(Array4<double>(rhs, v, ncomp_rhs), Array4<const double>(cons, mkbox(glo, ghi), h.tr.nvar()), dx, f,
			       Array4<const int>(redoFlag, v, 1), v);
}

// ------------------------------------------------------------------ multigroup helper functions (unit checks against independent formulas)
double orc_planck_integral(double x) { return planck::integrate_planck_from_0_to_x(x); }
double orc_planck_table_entry(int j) { return planck::Y_interp[j]; }

static auto mgSystem(int ngroups, double const *boundaries, double energy_unit, double k_B, double a_rad, double Erad_floor, int opacity_model) -> RadSystem
{
	RadSystem rs;
	rs.rt.nGroups = ngroups;
	rs.rt.radBoundaries.assign(boundaries, boundaries + ngroups + 1);
	rs.rt.energy_unit = energy_unit;
	rs.rt.radiation_constant = a_rad;
	rs.rt.Erad_floor = Erad_floor;
	rs.rt.opacity_model = opacity_model;
	rs.eos.tr.boltzmann_constant = k_B;
	return rs;
}
// ComputePlanckEnergyFractions / ComputeThermalRadiationMultiGroup (fractions, then E_g = max(a T^4 fraction_g, floor / nGroups))
void orc_planck_fractions(int ngroups, double const *boundaries, double energy_unit, double k_B, double a_rad, double Erad_floor, double T, double *fractions,
			  double *Erad_g)
{
	RadSystem const rs = mgSystem(ngroups, boundaries, energy_unit, k_B, a_rad, Erad_floor, 1);
	mg::MG const m(rs);
	auto const f = m.ComputePlanckEnergyFractions(m.boundaries(), T);
	auto const E = m.ComputeThermalRadiationMultiGroup(T, m.boundaries());
	for (int g = 0; g < ngroups; ++g) {
		fractions[g] = f[g];
		Erad_g[g] = E[g];
	}
}
double orc_planck_function(double energy_unit, double k_B, double a_rad, double nu, double T)
{
	double const b[2] = {1., 2.};
	RadSystem const rs = mgSystem(1, b, energy_unit, k_B, a_rad, 0., 1);
	return mg::MG(rs).PlanckFunction(nu, T);
}
void orc_group_mean_opacity(int ngroups, double const *boundaries, double const *expo, double const *lower, double const *alpha_quant, double *kappa)
{
	RadSystem const rs = mgSystem(ngroups, boundaries, 1., 1., 1., 0., 2);
	mg::MG const m(rs);
	mg::KappaExpoLower kel;
	kel.expo = mg::VA(ngroups + 1);
	kel.lower = mg::VA(ngroups + 1);
	mg::VA ratios(ngroups), alpha(ngroups);
	for (int g = 0; g < ngroups + 1; ++g) {
		kel.expo[g] = expo[g];
		kel.lower[g] = lower[g];
	}
	for (int g = 0; g < ngroups; ++g) {
		ratios[g] = boundaries[g + 1] / boundaries[g];
		alpha[g] = alpha_quant[g];
	}
	auto const k = m.ComputeGroupMeanOpacity(kel, ratios, alpha);
	for (int g = 0; g < ngroups; ++g) {
		kappa[g] = k[g];
	}
}
void orc_rad_quantity_exponents(int ngroups, double const *boundaries, double const *quant, double *exponents)
{
	RadSystem const rs = mgSystem(ngroups, boundaries, 1., 1., 1., 0., 3);
	mg::MG const m(rs);
	mg::VA q(ngroups);
	for (int g = 0; g < ngroups; ++g) {
		q[g] = quant[g];
	}
	auto const e = m.ComputeRadQuantityExponents(q, m.boundaries());
	for (int g = 0; g < ngroups; ++g) {
		exponents[g] = e[g];
	}
}

// ------------------------------------------------------------------ whole-simulation handle
struct orc_sim_config {
	int problem; // 0 = Sod, 1 = contact, 2 = Sedov
	int ndim;
	int n_cell[3];
	int max_grid_size[3];
	double prob_lo[3];
	double prob_hi[3];
	int periodic[3];
	// overrides (< 0 / NaN = keep the problem's default)
	double cfl;
	double stop_time;
	long max_timesteps;
	int reconstruction_order;
	int nscalars;
	// problem 3 (radiation-driven shell): the three columns of extern/dust_shell/initial_conditions.txt
	int table_len;
	double const *table_r, *table_Erad, *table_Frad;
	int rad_pow_mode; // RadTraits::pow_mode
	// problem 7 (parametrised 1-D hydro test): gamma, x_split, left[3], right[3], cfl, max_dt, init_dt, stop_time | profile, dirichlet
	double h1d[12];
	int h1d_i[2];
	double const *table_extra; // problem 17 (RadTube): fourth column of extern/pressure_tube/initial_conditions.txt (x, rho, Pgas, Erad)
	int opacity_model;	   // problems 16 / 18: OpacityModel override (<= 0: the problem file's choice)
};

// OpenMP team size for everything that follows (small problems run faster on one thread: every parallel region costs a barrier over
// the team, and a box that grants fewer CPUs than it shows makes an oversized team spin)
void orc_set_num_threads(int n)
{
#ifdef _OPENMP
	omp_set_num_threads(n > 0 ? n : 1);
#else
	(void)n;
#endif
}

void *orc_sim_create(orc_sim_config const *c)
{
	auto sim = std::make_unique<HydroSim>();
	setupGeometry(*sim, c->ndim, c->n_cell, c->prob_lo, c->prob_hi, c->periodic, c->max_grid_size);
	if (c->problem == 0) {
		setupSod(*sim);
	} else if (c->problem == 1) {
		setupContact(*sim, c->nscalars > 0 ? c->nscalars : 0);
	} else if (c->problem == 2) {
		setupSedov(*sim);
	} else if (c->problem == 3) {
		setupShell(*sim, c->table_len, c->table_r, c->table_Erad, c->table_Frad);
		sim->rad.rt.pow_mode = c->rad_pow_mode;
	} else if (c->problem == 8) {
		setupMatterCoupling(*sim);
		if (c->h1d[0] > 0) { // RadMatterCouplingRSLA (test_radiation_matter_coupling_rsla.cpp:22,43): c_hat = 0.1 c, nothing else differs
			sim->rad.rt.c_hat = c->h1d[0] * sim->rad.rt.c_light;
		}
		sim->rad.rt.pow_mode = c->rad_pow_mode;
	} else if (c->problem == 9) {
		setupSuOlson(*sim);
		sim->rad.rt.pow_mode = c->rad_pow_mode;
	} else if (c->problem == 7) {
		Hydro1DSpec p{};
		p.gamma = c->h1d[0];
		p.x_split = c->h1d[1];
		for (int n = 0; n < 3; ++n) {
			p.left[n] = c->h1d[2 + n];
			p.right[n] = c->h1d[5 + n];
		}
		p.cfl = c->h1d[8];
		p.max_dt = c->h1d[9];
		p.init_dt = c->h1d[10];
		p.stop_time = c->h1d[11];
		p.profile = c->h1d_i[0];
		p.dirichlet = c->h1d_i[1];
		p.max_timesteps = c->max_timesteps >= 0 ? c->max_timesteps : 100000;
		setupHydro1D(*sim, p);
	} else if (c->problem == 15) {
		setupShocktubeCMA(*sim);
	} else if (c->problem == 14) {
		setupRadPulse(*sim);
		sim->rad.rt.pow_mode = c->rad_pow_mode;
	} else if (c->problem == 13) {
		setupMarshakAsymptotic(*sim);
		sim->rad.rt.pow_mode = c->rad_pow_mode;
	} else if (c->problem == 12) {
		setupRadForce(*sim);
		sim->rad.rt.pow_mode = c->rad_pow_mode;
	} else if (c->problem == 11) {
		setupMarshak(*sim);
		sim->rad.rt.pow_mode = c->rad_pow_mode;
	} else if (c->problem == 10) {
		setupUniformAdvecting(*sim);
		sim->rad.rt.pow_mode = c->rad_pow_mode;
	} else if (c->problem >= 31 && c->problem <= 33) {
		setupAdvection(*sim, c->problem - 31);
	} else if (c->problem == 30) {
		setupGeneralOpacity(*sim);
		sim->rad.rt.pow_mode = c->rad_pow_mode;
	} else if (c->problem == 6) {
		setupScalarContact(*sim, c->nscalars > 0 ? c->nscalars : 1);
	} else if (c->problem == 5 || c->problem == 29) {
		setupStreaming(*sim, c->problem == 29 ? 1 : 0);
		sim->rad.rt.pow_mode = c->rad_pow_mode;
	} else if (c->problem == 4) {
		setupRadShock(*sim);
		sim->rad.rt.pow_mode = c->rad_pow_mode;
	} else if (c->problem == 16) {
		setupRadShockMG(*sim, c->opacity_model > 0 ? c->opacity_model : static_cast<int>(PPL_opacity_fixed_slope_spectrum));
		sim->rad.rt.pow_mode = c->rad_pow_mode;
	} else if (c->problem == 17) {
		setupRadTube(*sim, c->table_len, c->table_r, c->table_Erad, c->table_Frad, c->table_extra);
		sim->rad.rt.pow_mode = c->rad_pow_mode;
	} else if (c->problem == 18) {
		setupMarshakVaytet(*sim, c->opacity_model > 0 ? c->opacity_model : static_cast<int>(PPL_opacity_full_spectrum));
		sim->rad.rt.pow_mode = c->rad_pow_mode;
	} else if (c->problem == 25) {
		setupMarshakDust(*sim);
		sim->rad.rt.pow_mode = c->rad_pow_mode;
	} else if (c->problem == 23) {
		setupBlast2D(*sim);
	} else if (c->problem == 22) {
		setupQuirk(*sim);
	} else if (c->problem == 26 || c->problem == 27) { // h1d[1]: radiation.dust_gas_interaction_coeff of the deck
		setupLineCooling(*sim, c->problem == 27, c->h1d[1]);
		sim->rad.rt.pow_mode = c->rad_pow_mode;
	} else if (c->problem == 28) {
		setupMarshakDustPE(*sim, c->h1d[1]);
		sim->rad.rt.pow_mode = c->rad_pow_mode;
	} else if (c->problem == 21 || c->problem == 24) {
		setupRadDust(*sim, c->problem == 24);
		sim->rad.rt.pow_mode = c->rad_pow_mode;
	} else if (c->problem == 19 || c->problem == 20) {
		setupPulseMG(*sim, c->problem == 19);
		sim->rad.rt.pow_mode = c->rad_pow_mode;
	} else {
		return nullptr;
	}
	if ((c->problem == 4 || c->problem == 10) && c->h1d_i[0] > 0) {
		sim->rad.rt.beta_order = c->h1d_i[0]; // parity variants: the same problem with the O(beta^n) terms of another order
	}
	if (c->cfl > 0) {
		sim->cflNumber_ = c->cfl;
	}
	if (c->stop_time > 0) {
		sim->stopTime_ = c->stop_time;
	}
	if (c->max_timesteps >= 0) {
		sim->maxTimesteps_ = c->max_timesteps;
	}
	if (c->reconstruction_order > 0) {
		sim->reconstructionOrder_ = c->reconstruction_order;
	}
	return sim.release();
}

void orc_sim_destroy(void *p) { delete static_cast<HydroSim *>(p); }
int orc_sim_nboxes(void *p) { return static_cast<HydroSim *>(p)->state_new_cc_.size(); }
int orc_sim_ncomp(void *p) { return static_cast<HydroSim *>(p)->ncomp_cc; }
int orc_sim_nghost(void *p) { return static_cast<HydroSim *>(p)->nghost_cc; }
void orc_sim_box(void *p, int b, int lo[3], int hi[3])
{
	auto *s = static_cast<HydroSim *>(p);
	for (int d = 0; d < 3; ++d) {
		lo[d] = s->grids[b].lo[d];
		hi[d] = s->grids[b].hi[d];
	}
}
// copy the whole fab (valid + ghosts) of state_new_cc_ / state_old_cc_
void orc_sim_get_state(void *p, int which, int b, double *out)
{
	auto *s = static_cast<HydroSim *>(p);
	auto const &mf = (which == 0) ? s->state_new_cc_ : s->state_old_cc_;
	std::memcpy(out, mf.fabs[b].d.data(), mf.fabs[b].d.size() * sizeof(double));
}
void orc_sim_set_state(void *p, int which, int b, double const *in)
{
	auto *s = static_cast<HydroSim *>(p);
	auto &mf = (which == 0) ? s->state_new_cc_ : s->state_old_cc_;
	std::memcpy(mf.fabs[b].d.data(), in, mf.fabs[b].d.size() * sizeof(double));
}
void orc_sim_fill_ghosts(void *p, int which, double time)
{
	auto *s = static_cast<HydroSim *>(p);
	s->fillBC((which == 0) ? s->state_new_cc_ : s->state_old_cc_, time);
}
void orc_sim_set_rad_reconstruction_order(void *p, int order) { static_cast<HydroSim *>(p)->radiationReconstructionOrder_ = order; }
void orc_sim_set_wavespeed_correction(void *p, int on) { static_cast<HydroSim *>(p)->use_wavespeed_correction_ = (on != 0); }
double orc_sim_time(void *p) { return static_cast<HydroSim *>(p)->tNew_; }
double orc_sim_dt(void *p) { return static_cast<HydroSim *>(p)->dt_; }
long orc_sim_istep(void *p) { return static_cast<HydroSim *>(p)->istep; }
long orc_sim_cell_updates(void *p) { return static_cast<HydroSim *>(p)->cellUpdates_; }
double orc_sim_compute_dt(void *p)
{
	auto *s = static_cast<HydroSim *>(p);
	double const save = s->dt_;
	s->computeTimestep();
	double const r = s->dt_;
	s->dt_ = save;
	return r;
}
void orc_sim_counters(void *p, long out[3])
{
	auto *s = static_cast<HydroSim *>(p);
	out[0] = s->fofc1_cells;
	out[1] = s->fofc2_cells;
	out[2] = s->retries;
}
// the two transport stages of one radiation substep without the source terms (advanceRadiationForwardEuler + advanceRadiationMidpointRK2,
// QuokkaSimulation.hpp:1790-1857), state_old = state_new on entry as after swapRadiationState
void orc_sim_rad_transport_only(void *p, double dt_radiation)
{
	auto *s = static_cast<HydroSim *>(p);
	g_spacedim = s->ndim();
	s->advanceRadiationForwardEuler(s->tNew_, dt_radiation);
	s->advanceRadiationMidpointRK2(s->tNew_, dt_radiation);
}
// the fused, vectorised flux evaluation (hydro_fused.hpp) instead of the operator sequence: same bits (tests/test_oracle_fused_cpu.py)
// the floors of EnforceLimits (QuokkaSimulation.hpp densityFloor_, tempFloor_: 0 by default)
void orc_sim_set_limits(void *p, double densityFloor, double tempFloor)
{
	static_cast<HydroSim *>(p)->densityFloor_ = densityFloor;
	static_cast<HydroSim *>(p)->tempFloor_ = tempFloor;
}
// on: 0 operator form; 1 fused flux evaluation only; 3 whole stages box by box as well (HydroSim::fusedStage)
void orc_sim_set_fused_fluxes(void *p, int on)
{
	static_cast<HydroSim *>(p)->use_fused_fluxes = ((on & 1) != 0);
	static_cast<HydroSim *>(p)->use_fused_stages = ((on & 2) != 0);
}
// the carried form of the RK2 average (HydroSim::rk2_carry_rhs, this project's design: the GPU kernel's formula restated); 0 (default): the reference's
void orc_sim_set_rk2_carry_rhs(void *p, int on) { static_cast<HydroSim *>(p)->rk2_carry_rhs = (on != 0); }
long orc_sim_carry2_fallbacks(void *p) { return static_cast<HydroSim *>(p)->carry2_fallbacks; }
// what the last stage 1 of the carried form stored for box b, [ncomp + 1][valid cells] (S, then P(U_old)); returns the number of values, 0 before any
long orc_sim_carry_half(void *p, int b, double *out)
{
	auto *s = static_cast<HydroSim *>(p);
	if (s->carryHalf_.nc == 0) {
		return 0;
	}
	auto const &d = s->carryHalf_.fabs[b].d;
	std::copy(d.begin(), d.end(), out);
	return static_cast<long>(d.size());
}
// both forms of the flux evaluation on the sim's CURRENT state_new (ghost cells filled here): flux[d] as [6][faces] + face velocity [faces], x fastest
int orc_sim_hydro_fluxes(void *p, int fused, int b, int dir, double *flux_out, double *vel_out)
{
	auto *s = static_cast<HydroSim *>(p);
	s->fillBC(s->state_new_cc_, s->tNew_);
	bool const keep = s->use_fused_fluxes;
	s->use_fused_fluxes = (fused != 0);
	auto fv = s->computeHydroFluxes(s->state_new_cc_, s->ncompHydro());
	s->use_fused_fluxes = keep;
	auto const &F = fv.first[dir].fabs[b].d;
	auto const &V = fv.second[dir].fabs[b].d;
	std::copy(F.begin(), F.end(), flux_out);
	std::copy(V.begin(), V.end(), vel_out);
	return static_cast<int>(V.size());
}
// one coarse step with the reference's own dt control; returns 1 on success
int orc_sim_step(void *p)
{
	auto *s = static_cast<HydroSim *>(p);
	bool const ok = s->step();
	return ok ? 1 : 0;
}
// nsteps coarse steps, recording after each one the time and all components of the valid cell (i, j, k) of box b
// (what computeAfterTimestep of RadMatterCoupling collects); returns the number of steps taken
long orc_sim_run_record(void *p, long nsteps, int b, int i, int j, int k, double *out_t, double *out_u)
{
	auto *s = static_cast<HydroSim *>(p);
	long n = 0;
	double cur_time = s->tNew_;
	for (; n < nsteps && cur_time < s->stopTime_; ++n) {
		if (!s->step()) {
			break;
		}
		cur_time += s->dt_;
		s->tNew_ = cur_time;
		auto const a = s->state_new_cc_.const_array(b);
		out_t[n] = s->tNew_;
		for (int c = 0; c < s->ncomp_cc; ++c) {
			out_u[n * s->ncomp_cc + c] = a(i, j, k, c);
		}
		if (cur_time >= s->stopTime_ - 1.e-6 * s->dt_) {
			++n;
			break;
		}
	}
	return n;
}

// one hydro advance with a caller-supplied dt (no dt control): old <- new, advance
int orc_sim_advance_fixed_dt(void *p, double dt)
{
	auto *s = static_cast<HydroSim *>(p);
	g_spacedim = s->ndim();
	double const time = s->tNew_;
	s->dt_ = dt;
	s->tNew_ += dt;
	std::swap(s->state_old_cc_, s->state_new_cc_);
	bool const ok = s->advanceHydroAtLevelWithRetries(time, dt);
	++s->istep;
	s->cellUpdates_ += s->CountCells();
	return ok ? 1 : 0;
}
void orc_sim_rad_counters(void *p, long out[8])
{
	auto *s = static_cast<HydroSim *>(p);
	for (int n = 0; n < 4; ++n) {
		out[n] = s->rad_iteration_counter[n];
	}
	for (int n = 0; n < 3; ++n) {
		out[4 + n] = s->rad_iteration_failure_counter[n];
	}
	out[7] = s->radiationCellUpdates_;
}
// fills `out` (valid box of box b, 1 comp) with SetRadEnergySource at `time`
void orc_sim_rad_source(void *p, int b, double time, double *out)
{
	auto *s = static_cast<HydroSim *>(p);
	Array4<double> a(out, s->grids[b], 1);
	for (int64_t n = 0; n < s->grids[b].numPts(); ++n) {
		out[n] = 0.0;
	}
	if (s->SetRadEnergySource) {
		s->SetRadEnergySource(a, s->grids[b], s->geom, time);
	}
}
int orc_sim_evolve(void *p) { return static_cast<HydroSim *>(p)->evolve() ? 1 : 0; }

// ErrorEst of the gradient-threshold family on the (ghost-filled) new state of box b; `tags` covers the valid box, 1 char per cell
void orc_sim_tag_relative_gradient(void *p, int b, int field, double eta_threshold, double q_min, int min_inclusive, char *tags)
{
	auto *s = static_cast<HydroSim *>(p);
	Array4<char> t(tags, s->grids[b], 1);
	tagRelativeGradient(s->hydro, s->state_new_cc_.const_array(b), t, s->grids[b], s->ndim(), field, eta_threshold, q_min, min_inclusive != 0);
}

void orc_sim_tag_centered_gradient(void *p, int b, int comp, int dir, double dx, double eta_threshold, double q_min, int min_inclusive, char *tags)
{
	auto *s = static_cast<HydroSim *>(p);
	Array4<char> t(tags, s->grids[b], 1);
	tagCenteredGradient(s->state_new_cc_.const_array(b), t, s->grids[b], comp, dir, dx, eta_threshold, q_min, min_inclusive != 0);
}

// coarse -> fine interpolation of `region` (fine indices); arrays given with their lower / upper corners
void orc_interp_from_coarse(double *fine, const int *flo, const int *fhi, const double *crse_old, const double *crse_new, const int *clo, const int *chi,
			    int ncomp_total, const int *rlo, const int *rhi, double w_old, double w_new, int ncomp, int method, int hooks, int ndim, const int *ratio)
{
	Box fb, cb, region;
	for (int d = 0; d < 3; ++d) {
		fb.lo[d] = flo[d];
		fb.hi[d] = fhi[d];
		cb.lo[d] = clo[d];
		cb.hi[d] = chi[d];
		region.lo[d] = rlo[d];
		region.hi[d] = rhi[d];
	}
	Array4<double> f(fine, fb, ncomp_total);
	Array4<const double> co(crse_old, cb, ncomp_total), cn(crse_new, cb, ncomp_total);
	interpFromCoarse(f, co, cn, region, w_old, w_new, ncomp, method, hooks != 0, ndim, ratio);
}

// amrex::average_down of one fine array onto one coarse array; boxes as lo[3], hi[3] (with ghosts = the arrays' extents); region in coarse indices
void orc_average_down(const double *fine, const int *flo, const int *fhi, double *crse, const int *clo, const int *chi, int ncomp_total, const int *rlo,
		      const int *rhi, int scomp, int ncomp, const int *ratio)
{
	Box fb, cb, region;
	for (int d = 0; d < 3; ++d) {
		fb.lo[d] = flo[d];
		fb.hi[d] = fhi[d];
		cb.lo[d] = clo[d];
		cb.hi[d] = chi[d];
		region.lo[d] = rlo[d];
		region.hi[d] = rhi[d];
	}
	Array4<const double> f(fine, fb, ncomp_total);
	Array4<double> c(crse, cb, ncomp_total);
	averageDown(f, c, region, scomp, ncomp, ratio);
}

// ------------------------------------------------------------------ tabulated cooling (cooling.hpp)
// the five datasets of a cloudy_cooling_tools file as H5Dread delivers them (Parameter1[n0], Temperature[n1], Cooling / Heating / MMW [n0][n1])
void *orc_cloudy_create(int n0, int n1, const double *parameter1, const double *temperature, const double *cooling_rate, const double *heating_rate, const double *mmw)
{
	return new cooling::cloudy_tables(cooling::prepare_tables(n0, n1, parameter1, temperature, cooling_rate, heating_rate, mmw));
}
void orc_cloudy_destroy(void *p) { delete static_cast<cooling::cloudy_tables *>(p); }
// out: T_min, T_max, mmw_min, mmw_max
void orc_cloudy_ranges(void *p, double *out)
{
	auto const &t = *static_cast<cooling::cloudy_tables *>(p);
	out[0] = t.T_min;
	out[1] = t.T_max;
	out[2] = t.mmw_min;
	out[3] = t.mmw_max;
}
// the prepared arrays: which = 0 log_nH, 1 log_Tgas, 2 cooling, 3 heating, 4 mean molecular weight (n_H fastest)
void orc_cloudy_get(void *p, int which, double *out)
{
	auto const &t = *static_cast<cooling::cloudy_tables *>(p);
	std::vector<double> const *v[5] = {&t.log_nH_v, &t.log_Tgas_v, &t.cool_v, &t.heat_v, &t.mmw_v};
	std::copy(v[which]->begin(), v[which]->end(), out);
}
// what: 0 ComputeTgasFromEgas, 1 ComputeEgasFromTgas, 2 ComputeMMW, 3 ComputeCoolingLength, 4 cloudy_cooling_function (val = E_int, T, E_int, E_int, T)
void orc_cloudy_evaluate(void *p, double gamma, int what, long n, const double *rho, const double *val, double *out)
{
	auto const &t = *static_cast<cooling::cloudy_tables *>(p);
	_Pragma("omp parallel for schedule(dynamic, 64)")
	for (long i = 0; i < n; ++i) {
		switch (what) {
		case 0:
			out[i] = cooling::ComputeTgasFromEgas(rho[i], val[i], gamma, t);
			break;
		case 1:
			out[i] = cooling::ComputeEgasFromTgas(rho[i], val[i], gamma, t);
			break;
		case 2:
			out[i] = cooling::ComputeMMW(rho[i], val[i], gamma, t);
			break;
		case 3:
			out[i] = cooling::ComputeCoolingLength(rho[i], val[i], gamma, t);
			break;
		default:
			out[i] = cooling::cloudy_cooling_function(rho[i], val[i], t);
			break;
		}
	}
}
// computeCooling over n cells: U[6][n] = (rho, x1Mom, x2Mom, x3Mom, Egas, Eint_aux), component outermost; nsteps[n]
void orc_cloudy_compute_cooling(void *p, double gamma, double dt, double T_floor, long n, double *U, int *nsteps)
{
	auto const &t = *static_cast<cooling::cloudy_tables *>(p);
	_Pragma("omp parallel for schedule(dynamic, 16)")
	for (long i = 0; i < n; ++i) {
		double cell[6];
		for (int c = 0; c < 6; ++c) {
			cell[c] = U[c * n + i];
		}
		nsteps[i] = cooling::computeCoolingCell(cell, dt, t, T_floor, gamma);
		U[4 * n + i] = cell[4];
		U[5 * n + i] = cell[5];
	}
}
// which libm the per-cell functions call from now on: 0 glibc (the default), 1 portable_libm.hpp (cooling.hpp, the hook); not to be changed while
// another thread evaluates
void orc_cloudy_set_libm(int mode) { cooling::libm_mode() = mode; }
// portable_libm.hpp itself: which = 0 log10, 1 x^(-1/2)
void orc_portable_libm(int which, long n, const double *x, double *out)
{
	for (long i = 0; i < n; ++i) {
		out[i] = (which == 0) ? portable_libm::log10_portable(x[i]) : portable_libm::rsqrt_portable(x[i]);
	}
}
// orc_cloudy_compute_cooling with a record per cell, rec[6][n]: attempts, refused attempts, deepest retry, failed right-hand sides, function
// evaluations of Algorithm 748, branch mask (cooling.hpp: BR_*)
void orc_cloudy_cooling_cells(void *p, double gamma, double dt, double T_floor, long n, double *U, int *nsteps, int *rec)
{
	auto const &t = *static_cast<cooling::cloudy_tables *>(p);
	_Pragma("omp parallel for schedule(dynamic, 16)")
	for (long i = 0; i < n; ++i) {
		double cell[6];
		for (int c = 0; c < 6; ++c) {
			cell[c] = U[c * n + i];
		}
		cooling::cell_record r;
		cooling::record() = &r;
		nsteps[i] = cooling::computeCoolingCell(cell, dt, t, T_floor, gamma);
		cooling::record() = nullptr;
		U[4 * n + i] = cell[4];
		U[5 * n + i] = cell[5];
		const int fields[6] = {r.attempts, r.refused, r.deepest_retry, r.failed_rhs, r.f_evals, static_cast<int>(r.mask)};
		for (int c = 0; c < 6; ++c) {
			rec[c * n + i] = fields[c];
		}
	}
}

// ------------------------------------------------------------------ the matter-radiation exchange, cell by cell
// The radiation and EOS traits of one single-group problem as a closed set: the fields of qk_rad_traits / qk_hydro_traits (include/quokka_amd.h)
// the exchange reads.  gamma == 1: isothermal.
struct orc_rad_cell_traits {
	double c_light, c_hat, radiation_constant, Erad_floor;
	double kappaP, kappaE, kappaF;
	double opacity_T_ref, opacity_T_exponent, opacity_pow_floor;
	double gamma, mean_molecular_weight, boltzmann_constant;
	int beta_order, opacity_model, pow_mode, eddington_model;
};

// the three opacity hooks as the closed set of qk_rad_traits::opacity_model (0: constant, 1: k0 / rho, 2: k0 max((T / T_ref)^p, floor) / rho);
// pow_mode 1: the exponents 3, -3 and -3.5 as products and square roots, as in setupMarshakAsymptotic / setupRadPulse (problems.hpp)
static auto closedOpacity(orc_rad_cell_traits const &t, double k0) -> std::function<double(double, double)>
{
	if (t.opacity_model == 0) {
		return [k0](double, double) { return k0; };
	}
	if (t.opacity_model == 1) {
		return [k0](double rho, double) { return k0 / rho; };
	}
	const double T_ref = t.opacity_T_ref, p = t.opacity_T_exponent, floor = t.opacity_pow_floor;
	const int pow_mode = t.pow_mode;
	return [=](double rho, double T) {
		const double x = T / T_ref;
		double pw = NAN;
		if (pow_mode == 1 && p == 3.0) {
			pw = (x * x) * x;
		} else if (pow_mode == 1 && p == -3.0) {
			pw = 1.0 / ((x * x) * x);
		} else if (pow_mode == 1 && p == -3.5) {
			pw = 1.0 / (((x * x) * x) * std::sqrt(x));
		} else {
			pw = std::pow(x, p);
		}
		return (k0 * ((pw > floor) ? pw : floor)) / rho;
	};
}

// AddSourceTermsSingleGroup on each of n cells as a box of its own.  U[10][n] (component outermost) is updated in place, src[n] is the radiation
// energy source.  per_cell[5][n]: solves, Newton iterations summed over the solves (n + 1 per solve, the counter's convention), the largest
// n + 1 of one solve, Newton failures, outer-iteration failures.  totals[7]: p_iteration_counter[0..3] then p_iteration_failure_counter[0..2].
void orc_rad_source_cells(orc_rad_cell_traits const *t, long n, double *U, double const *src, double dt_radiation, int stage, int *per_cell, long *totals)
{
	RadSystem rs;
	rs.rt.c_light = t->c_light;
	rs.rt.c_hat = t->c_hat;
	rs.rt.radiation_constant = t->radiation_constant;
	rs.rt.Erad_floor = t->Erad_floor;
	rs.rt.beta_order = t->beta_order;
	rs.rt.pow_mode = t->pow_mode;
	rs.rt.eddington_model = t->eddington_model;
	rs.eos.tr.gamma = t->gamma;
	rs.eos.tr.mean_molecular_weight = t->mean_molecular_weight;
	rs.eos.tr.boltzmann_constant = t->boltzmann_constant;
	rs.nstartHyperbolic_ = 6;
	rs.ndim = 3;
	rs.ComputePlanckOpacity = closedOpacity(*t, t->kappaP);
	rs.ComputeEnergyMeanOpacity = closedOpacity(*t, t->kappaE);
	rs.ComputeFluxMeanOpacity = closedOpacity(*t, t->kappaF);
	long tot[7] = {0, 0, 0, 0, 0, 0, 0};
	Box one; // lo = hi = (0, 0, 0)
	_Pragma("omp parallel")
	{
		long mine[7] = {0, 0, 0, 0, 0, 0, 0};
		_Pragma("omp for schedule(dynamic, 64)")
		for (long i = 0; i < n; ++i) {
			double cell[10];
			for (int c = 0; c < 10; ++c) {
				cell[c] = U[c * n + i];
			}
			int it[4] = {0, 0, 0, 0}, fail[3] = {0, 0, 0};
			rs.AddSourceTermsSingleGroup(Array4<double>(cell, one, 10), Array4<const double>(src + i, one, 1), one, dt_radiation, stage, it, fail);
			for (int c = 0; c < 10; ++c) {
				U[c * n + i] = cell[c];
			}
			per_cell[0 * n + i] = it[0];
			per_cell[1 * n + i] = it[1];
			per_cell[2 * n + i] = it[2];
			per_cell[3 * n + i] = fail[0];
			per_cell[4 * n + i] = fail[2];
			mine[0] += it[0];
			mine[1] += it[1];
			mine[2] = std::max(mine[2], static_cast<long>(it[2]));
			mine[3] += it[3];
			for (int c = 0; c < 3; ++c) {
				mine[4 + c] += fail[c];
			}
		}
		_Pragma("omp critical")
		for (int c = 0; c < 7; ++c) {
			tot[c] = (c == 2) ? std::max(tot[c], mine[c]) : tot[c] + mine[c];
		}
	}
	for (int c = 0; c < 7; ++c) {
		totals[c] = tot[c];
	}
}

// ------------------------------------------------------------------ the multigroup matter-radiation exchange, cell by cell
// The fields of qk_rad_traits / qk_hydro_traits (include/quokka_amd.h) the multigroup exchange reads, as a closed set.  gamma == 1: isothermal.
struct orc_rad_mg_cell_traits {
	double c_light, c_hat, radiation_constant, Erad_floor;
	double energy_unit;
	double rad_boundaries[9], mg_kappa_exponent[9], mg_kappa_lower[9];
	double mg_kappa_rho_exponent, mg_kappa_T_ref, mg_kappa_T_exponent;
	double dust_gas_interaction_coeff, gas_dust_coupling_threshold;
	double cooling_linear_coeff[8], cr_heating_rate, pe_heating_E1_derivative;
	double gamma, mean_molecular_weight, boltzmann_constant;
	int beta_order, eddington_model, pow_mode, ngroups, mg_opacity_model;
	int enable_dust_gas_thermal_coupling_model, thermal_model, enable_photoelectric_heating;
};

// seed == 0 (the default): the multigroup path calls libm as it is.  Otherwise the results of pow, exp, log and log10 in radiation_multigroup.hpp
// (the Planck-integral lookup included) and in the opacity hook below are moved by up to `ulps` ulps (radiation_multigroup.hpp, namespace diag).
// Single-group radiation, cooling and hydro never see it.
void orc_set_libm_jitter(unsigned long long seed, int ulps)
{
	diag::jitter_seed = seed;
	diag::jitter_ulps = ulps;
}

// AddSourceTermsMultiGroup on each of n cells as a box of its own.  U[6 + 4 ng][n] (component outermost) is updated in place, src[ng][n] is the
// radiation energy source.  per_cell[8][n]: solves, Newton iterations summed over the solves (n + 1 per solve), the largest n + 1 of one solve,
// Newton failures, outer-iteration failures, negative dust temperatures, decoupled solves, the branch mask (diag::Branch).
// totals[7]: p_iteration_counter[0..3] then p_iteration_failure_counter[0..2], the layout of the C-ABI.
void orc_rad_mg_source_cells(orc_rad_mg_cell_traits const *t, long n, double *U, double const *src, double dt_radiation, int stage, int *per_cell, long *totals)
{
	RadSystem rs;
	rs.rt.c_light = t->c_light;
	rs.rt.c_hat = t->c_hat;
	rs.rt.radiation_constant = t->radiation_constant;
	rs.rt.Erad_floor = t->Erad_floor;
	rs.rt.beta_order = t->beta_order;
	rs.rt.pow_mode = t->pow_mode;
	rs.rt.eddington_model = t->eddington_model;
	rs.rt.nGroups = t->ngroups;
	rs.rt.opacity_model = t->mg_opacity_model;
	rs.rt.energy_unit = t->energy_unit;
	rs.rt.radBoundaries.assign(t->rad_boundaries, t->rad_boundaries + t->ngroups + 1);
	rs.rt.enable_dust_gas_thermal_coupling_model = (t->enable_dust_gas_thermal_coupling_model != 0);
	rs.rt.dustGasInteractionCoeff = t->dust_gas_interaction_coeff;
	rs.rt.gas_dust_coupling_threshold = t->gas_dust_coupling_threshold;
	rs.rt.thermal_model = t->thermal_model;
	rs.rt.enable_photoelectric_heating = (t->enable_photoelectric_heating != 0);
	rs.eos.tr.gamma = t->gamma;
	rs.eos.tr.mean_molecular_weight = t->mean_molecular_weight;
	rs.eos.tr.boltzmann_constant = t->boltzmann_constant;
	rs.nstartHyperbolic_ = 6;
	rs.ndim = 3;
	const int ng = t->ngroups;
	const orc_rad_mg_cell_traits tr = *t;
	// include/quokka_amd.h: exponent[g] = mg_kappa_exponent[g]; lower_value[g] = mg_kappa_lower[g] * pow(rho, a) * pow(T / T_ref, b), either power
	// with exponent 0 skipped, exponent -1 on rho a division
	rs.DefineOpacityExponentsAndLowerValues = [tr, ng](double const *, double rho, double T, double *expo, double *lower) {
		for (int g = 0; g < ng + 1; ++g) {
			expo[g] = tr.mg_kappa_exponent[g];
			double v = tr.mg_kappa_lower[g];
			if (tr.mg_kappa_rho_exponent == -1.0) {
				v = v / rho;
			} else if (tr.mg_kappa_rho_exponent != 0.0) {
				v = v * diag::pow(rho, tr.mg_kappa_rho_exponent);
			}
			if (tr.mg_kappa_T_exponent != 0.0) {
				v = v * diag::pow(T / tr.mg_kappa_T_ref, tr.mg_kappa_T_exponent);
			}
			lower[g] = v;
		}
	};
	// include/quokka_amd.h, the ISM hooks: DefineNetCoolingRate(T, n)[g] = cooling_linear_coeff[g] * T (its temperature derivative the coefficient),
	// DefineCosmicRayHeatingRate(n) = cr_heating_rate, DefinePhotoelectricHeatingE1Derivative(T, n) = pe_heating_E1_derivative
	rs.DefineNetCoolingRate = [tr, ng](double T, double, double *out) {
		for (int g = 0; g < ng; ++g) {
			out[g] = tr.cooling_linear_coeff[g] * T;
		}
	};
	rs.DefineNetCoolingRateTempDerivative = [tr, ng](double, double, double *out) {
		for (int g = 0; g < ng; ++g) {
			out[g] = tr.cooling_linear_coeff[g];
		}
	};
	rs.DefineCosmicRayHeatingRate = [tr](double) { return tr.cr_heating_rate; };
	rs.DefinePhotoelectricHeatingE1Derivative = [tr](double, double) { return tr.pe_heating_E1_derivative; };
	mg::MG const m(rs);
	const int nc = 6 + 4 * ng;
	long tot[7] = {0, 0, 0, 0, 0, 0, 0};
	Box one; // lo = hi = (0, 0, 0)
	_Pragma("omp parallel")
	{
		long mine[7] = {0, 0, 0, 0, 0, 0, 0};
		_Pragma("omp for schedule(dynamic, 64)")
		for (long i = 0; i < n; ++i) {
			double cell[6 + 4 * 8], s[8];
			for (int c = 0; c < nc; ++c) {
				cell[c] = U[c * n + i];
			}
			for (int g = 0; g < ng; ++g) {
				s[g] = src[g * n + i];
			}
			int it[4] = {0, 0, 0, 0}, fail[3] = {0, 0, 0};
			diag::mask = 0;
			m.AddSourceTermsMultiGroup(Array4<double>(cell, one, nc), Array4<const double>(s, one, ng), one, dt_radiation, stage, it, fail);
			for (int c = 0; c < nc; ++c) {
				U[c * n + i] = cell[c];
			}
			per_cell[0 * n + i] = it[0];
			per_cell[1 * n + i] = it[1];
			per_cell[2 * n + i] = it[2];
			per_cell[3 * n + i] = fail[0];
			per_cell[4 * n + i] = fail[2];
			per_cell[5 * n + i] = fail[1];
			per_cell[6 * n + i] = it[3];
			per_cell[7 * n + i] = static_cast<int>(diag::mask);
			mine[0] += it[0];
			mine[1] += it[1];
			mine[2] = std::max(mine[2], static_cast<long>(it[2]));
			mine[3] += it[3];
			for (int c = 0; c < 3; ++c) {
				mine[4 + c] += fail[c];
			}
		}
		_Pragma("omp critical")
		for (int c = 0; c < 7; ++c) {
			tot[c] = (c == 2) ? std::max(tot[c], mine[c]) : tot[c] + mine[c];
		}
	}
	for (int c = 0; c < 7; ++c) {
		totals[c] = tot[c];
	}
}

// ------------------------------------------------------------------ the radiation transport operators, face by face and stage by stage
// Of orc_rad_cell_traits these read c_light, c_hat, Erad_floor and eddington_model.
static auto transportSystem(orc_rad_cell_traits const *t, int ngroups, int ndim, int nstart) -> RadSystem
{
	RadSystem rs;
	rs.rt.c_light = t->c_light;
	rs.rt.c_hat = t->c_hat;
	rs.rt.Erad_floor = t->Erad_floor;
	rs.rt.eddington_model = t->eddington_model;
	rs.rt.nGroups = ngroups;
	rs.nstartHyperbolic_ = nstart;
	rs.ndim = ndim;
	return rs;
}

// ConservedToPrimitive (radiation_system.hpp:589-614) on n cells of one group: cons[4][n] -> prim[4][n], component outermost
void orc_rad_cons_to_prim(orc_rad_cell_traits const *t, long n, double const *cons, double *prim)
{
	RadSystem const rs = transportSystem(t, 1, 1, 0);
	Box row;
	row.hi[0] = static_cast<int>(n) - 1;
	rs.ConservedToPrimitive(Array4<const double>(cons, row, 4), Array4<double>(prim, row, 4), row);
}

// ComputeFluxes<dir[f]> (radiation_system.hpp:985-1139) on each of n faces as a box of one face: pL / pR the reconstructed primitive states,
// consL / consR the conserved states of the two cells, eps the factor S_corr of the face (1: no wavespeed correction); all [4][n], component
// outermost.  F[4][n] receives the flux, mask[n] tdiag::Face.
void orc_rad_face_fluxes(orc_rad_cell_traits const *t, long n, int const *dir, double const *pL, double const *pR, double const *consL, double const *consR,
			 double const *eps, double *F, int *mask)
{
	g_spacedim = 3;
	RadSystem const rs = transportSystem(t, 1, 3, 0);
	_Pragma("omp parallel for schedule(static)")
	for (long f = 0; f < n; ++f) {
		int const d = dir[f];
		Box face; // lo = hi = (0, 0, 0): the face between cells -1 and 0 along d
		Box cells;
		cells.lo[d] = -1;
		double l[4], r[4], U[8], e = eps[f], flux[4], diffusive[4];
		for (int c = 0; c < 4; ++c) {
			l[c] = pL[c * n + f];
			r[c] = pR[c * n + f];
			U[2 * c] = consL[c * n + f]; // (two cells along d, component outermost)
			U[2 * c + 1] = consR[c * n + f];
		}
		int m = 0;
		Array4<const double> const epsA(&e, face, 1);
		Array4<int> const maskA(&m, face, 1);
		rs.ComputeFluxes(d, Array4<double>(flux, face, 4), Array4<double>(diffusive, face, 4), Array4<const double>(l, face, 4), Array4<const double>(r, face, 4),
				 face, Array4<const double>(U, cells, 4), nullptr, false, &epsA, &maskA);
		for (int c = 0; c < 4; ++c) {
			F[c * n + f] = flux[c];
		}
		mask[f] = m;
	}
}

// One transport stage of one box on arrays the caller owns and has ghost-filled (nghost cells in the first ndim directions, 6 + 4 ngroups
// components): computeRadiationFluxes (QuokkaSimulation.hpp:1884-1961: ConservedToPrimitive, the reconstruction of `order`, ComputeFluxes per
// direction) of U_in, then PredictStep(U0 -> U_new) (stage 1) or AddFluxesRK2(U_new; U0, U1 = U_in; the old-state fluxes, of weight 0.5 - IMEX_a32
// = 0, are those of U0) (stage 2).  eps[d]: NULL or S_corr per face and group; flux[d] / fmask[d]: the face arrays of direction d (4 ngroups /
// ngroups components), cmask: the valid box, ngroups components.  U_new: only the radiation components of the valid cells are written.
void orc_rad_transport_stage(orc_rad_cell_traits const *t, int ngroups, int ndim, int order, int stage, double const *U_in, double const *U0, double *U_new,
			     int const vlo[3], int const vhi[3], int nghost, double dt, double const dx[3], double const *const eps[3], double *const flux[3],
			     int *const fmask[3], int *cmask)
{
	g_spacedim = ndim;
	RadSystem const rs = transportSystem(t, ngroups, ndim, 6);
	int const nvars = rs.nRadComps(), ncomp = 6 + nvars;
	Box const indexRange = mkbox(vlo, vhi);
	Box const ghostRange = grow(indexRange, nghost, ndim);
	auto fluxesOf = [&](double const *U, bool record) {
		Array4<const double> const consVar(U, ghostRange, ncomp);
		std::array<Fab<double>, 3> out;
		for (int dir = 0; dir < ndim; ++dir) {
			Box const reconstructRange = grow(indexRange, 1, ndim);
			Box const x1ReconstructRange = faceBox(reconstructRange, dir);
			Fab<double> primVar(ghostRange, nvars);
			Fab<double> x1LeftState(x1ReconstructRange, nvars);
			Fab<double> x1RightState(x1ReconstructRange, nvars);
			rs.ConservedToPrimitive(consVar, primVar.array(), ghostRange);
			if (order == 3) {
				ReconstructStatesPPM(dir, primVar.const_array(), x1LeftState.array(), x1RightState.array(), reconstructRange, nvars);
			} else if (order == 2) {
				ReconstructStatesPLM(dir, lim_MC, primVar.const_array(), x1LeftState.array(), x1RightState.array(), x1ReconstructRange, nvars);
			} else {
				ReconstructStatesConstant(dir, primVar.const_array(), x1LeftState.array(), x1RightState.array(), x1ReconstructRange, nvars);
			}
			Box const x1FluxRange = faceBox(indexRange, dir);
			out[dir] = Fab<double>(x1FluxRange, nvars);
			Fab<double> diffusive(x1FluxRange, nvars);
			Fab<int> took(x1FluxRange, ngroups);
			Array4<const double> const epsA((eps != nullptr && eps[dir] != nullptr) ? eps[dir] : nullptr, x1FluxRange, ngroups);
			Array4<int> const tookA = took.array();
			rs.ComputeFluxes(dir, out[dir].array(), diffusive.array(), x1LeftState.const_array(), x1RightState.const_array(), x1FluxRange, consVar, nullptr,
					 false, (epsA.p != nullptr) ? &epsA : nullptr, &tookA);
			if (record) {
				std::copy(out[dir].d.begin(), out[dir].d.end(), flux[dir]);
				std::copy(took.d.begin(), took.d.end(), fmask[dir]);
			}
		}
		return out;
	};
	auto const fl = fluxesOf(U_in, true);
	std::array<Array4<const double>, 3> f{};
	for (int d = 0; d < ndim; ++d) {
		f[d] = fl[d].const_array();
	}
	Array4<int> const cellMask(cmask, indexRange, ngroups);
	Array4<double> const out(U_new, ghostRange, ncomp);
	if (stage == 1) {
		rs.PredictStep(Array4<const double>(U0, ghostRange, ncomp), out, f, dt, dx, indexRange, &cellMask);
	} else {
		auto const flOld = fluxesOf(U0, false);
		std::array<Array4<const double>, 3> f0{};
		for (int d = 0; d < ndim; ++d) {
			f0[d] = flOld[d].const_array();
		}
		// (U_new may be the array of U_in, as in the driver: AddFluxesRK2 reads U1 and writes U_new at the same cell only)
		rs.AddFluxesRK2(out, Array4<const double>(U0, ghostRange, ncomp), Array4<const double>(U_in, ghostRange, ncomp), f0, f, dt, dx, indexRange, &cellMask);
	}
}

} // extern "C"
