/*
 * libmslice -- C ABI of the MI355X (gfx950) multislice engine.
 *
 * This is the drop-in boundary of the hot path.  The reference (h-walk/PySlice) has no
 * native layer: its path is Python calling torch/numpy ops.  Every entry point below
 * therefore replaces the *body* of one reference Python function; the reference-side
 * binding a maintainer would add is the ctypes stub shown in INTEGRATION.md.
 *
 * Conventions
 *   - plain C types only; every function returns 0 on success or a negative msl_status;
 *     no C++ exception crosses the ABI; msl_last_error() gives the message.
 *   - caller owns every host buffer; the library owns all device buffers for the life of
 *     the handle and keeps no host pointer after a call returns.
 *   - one handle == one HIP device + one HIP stream; a handle is not thread-safe, distinct
 *     handles (one per GPU / per process) are independent.
 *   - arithmetic is complex64 / float32 on the device ("c64" below = interleaved float
 *     re,im).  Setup scalars are taken as double and reduced on the host.
 *   - wave-function layout everywhere: [probe][x][y] with y fastest (reference axis order,
 *     src/multislice/multislice.py:285-294).
 */
#ifndef MSLICE_H
#define MSLICE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MSL_ABI_VERSION 3   /* 2: reduction / streaming entry points and enum values added in rounds 2-3;
                              * 3: line-aligned pixel pitch of the result buffers (msl_result_pitch), `ld` argument of the reductions */

typedef struct msl_handle msl_handle;

typedef enum {
    MSL_OK = 0,
    MSL_ERR_INVALID = -1,     /* bad argument / shape (Python wrapper raises ValueError)   */
    MSL_ERR_HIP = -2,         /* HIP runtime failure (RuntimeError)                        */
    MSL_ERR_UNSUPPORTED = -3, /* e.g. grid length with a prime factor the FFT cannot do    */
    MSL_ERR_STATE = -4,       /* call order violated (e.g. propagate before potential)     */
    MSL_ERR_NOMEM = -5
} msl_status;

/* Grid + beam description.  Replaces the scalars MultisliceCalculator.setup() derives
 * (src/multislice/calculators.py:144-161) and Propagate() derives
 * (src/multislice/multislice.py:258-275). */
typedef struct {
    int32_t nx, ny, nz;        /* grid: len(xs), len(ys), number of slices                 */
    double  dx, dy;            /* xs[1]-xs[0], ys[1]-ys[0]   (potentials.py:228-229)       */
    double  dz;                /* slice spacing used by the Fresnel propagator (multislice.py:266) */
    double  wavelength;        /* Angstrom           (multislice.py:41-42)                 */
    double  sigma;             /* interaction parameter (multislice.py:258-260)            */
    int32_t n_probes;          /* P                                                         */
    int32_t n_frames;          /* T_local: frame slots of the (P,T_local,nx,ny) result; 0 = no result buffer */
    int32_t device;            /* HIP device ordinal                                        */
    int32_t keep_potential;    /* 1: also keep V (nz,nx,ny) float32 for msl_download(MSL_BUF_POTENTIAL) */
    int32_t fft_path;          /* 0 = auto (fast kernels when the size allows), 1 = generic LDS Stockham only */
    int32_t window_nx, window_ny; /* k-window (not in the reference, which keeps every pixel: calculators.py:161):
                                * keep only the central window_nx x window_ny pixels of each fftshifted exit-wave spectrum,
                                * rows [nx/2 - window_nx/2, +window_nx), columns likewise; the result, intensity and frame
                                * buffers then have shape (.., window_nx, window_ny).  0 = the full axis. */
    int32_t launch_timing;     /* 1: record a HIP event after every slice-loop launch so that msl_get_counters reports per-kernel
                                * launch counts and durations (bench.py's roofline); 0: no events (production) */
    int32_t frame_batch;       /* B > 1: up to B MD frames share every slice-loop launch (image index = frame * P + probe, each frame with
                                * its own transmission stack): the single-probe default of the reference (calculators.py:152-153) is
                                * otherwise launch-bound.  Potentials are built into batch slots (msl_select_batch_slot) and run by
                                * msl_propagate_frames.  Costs B x the work buffers and transmission stacks.  0 / 1 = off; ignored
                                * (treated as 1) with keep_potential. */
    int32_t bin_nx, bin_ny;    /* detector binning: every stored pixel is the sum of bin_nx x bin_ny neighbouring pixels of the
                                * fftshifted spectrum (of the k-window, when there is one; the window must be a multiple of the bin).  The
                                * result, intensity and frame buffers then have shape (.., wx/bin_nx, wy/bin_ny).  0 / 1 = off. */
    int32_t reserved[1];
} msl_config;

typedef enum {
    MSL_BUF_PROBES = 0,        /* (P,nx,ny) c64     initial probes psi_0                    */
    MSL_BUF_EXIT = 1,          /* (P,nx,ny) c64     real-space exit waves of the last msl_propagate */
    MSL_BUF_POTENTIAL = 2,     /* (nz,nx,ny) f32    V of the last msl_build_potential (slice-major!) */
    MSL_BUF_TRANSMISSION = 3,  /* (nz,nx,ny) c64    exp(i sigma V)                           */
    MSL_BUF_WAVEFUNCTION = 4,  /* (P,T_local,pitch) c64  fftshift(fft2(exit)) per frame slot: wx*wy pixels (wx,wy = nx,ny or the
                                *                    k-window) at a pitch of msl_result_pitch() pixels, the rest of a row is zero */
    MSL_BUF_INTENSITY = 5,     /* (P,T,pitch) f32   TACAW |FFT_t|^2 of the last msl_tacaw (same pitch; after a stream: pitch = wx*wy) */
    MSL_BUF_FORMFACTOR = 6,    /* (n_species,nx,ny) f32 Kirkland f_Z(q^2) of the last potential build */
    /* streaming TACAW, while a stream is open (msl_tacaw_stream_begin .. _finish): the partial sums of this handle, for the
     * caller's collective when the frames of a run are sharded over several handles / processes (msl_device_ptr only) */
    MSL_BUF_STREAM_ACC = 7,    /* (P,n_bins,K) c64  sum_t (Psi[p,t,k] - ref[p,k]) exp(-2 pi i u t / T) over the frames pushed so far */
    MSL_BUF_STREAM_S1 = 8,     /* (P,K) 2 x f64     sum_t Psi */
    MSL_BUF_STREAM_S2 = 9,     /* (P,K) f64         sum_t |Psi|^2 */
    MSL_BUF_STREAM_REF = 10,   /* (P,K) c64         the reference pattern (msl_tacaw_stream_set_reference), NULL when none is set */
    MSL_BUF_LAYERS = 11,       /* (L,P,T_local,pitch) c64  the spectra of every layer (msl_set_layers), the exit wave last; L = 1 without
                                *                    layers (then the same memory as MSL_BUF_WAVEFUNCTION) */
    MSL_BUF_SMATRIX = 12,      /* (Bm,nx,ny) c64    the PRISM S-matrix of the last msl_smatrix_build: the exit waves of the Bm beams */
    MSL_BUF_FORMFACTOR_ABS = 13, /* (n_species,nx,ny) f32 the absorptive tables g of the last build with msl_set_absorption(.., absorb != 0) */
    MSL_BUF_ABSORPTION = 14,   /* (nz,nx,ny) f32    Omega of the last build with msl_set_absorption(.., absorb != 0) */
    MSL_BUF_FORMFACTOR_TDS = 15, /* (n_det,n_species,nx,ny) f32 the detector-restricted tables g_det of the last build with msl_set_tds */
    MSL_BUF_TDS_WEIGHT = 16,   /* (n_det,nz,nx,ny) f32 the TDS weights w = 1 - exp(-2 sigma^2 Omega_det) of the last build with msl_set_tds */
    MSL_BUF_FORMFACTOR_FINITE = 17, /* (n_species*(2R+1)*J,nx,ny) f32 the channel tables F_Z(k; alpha, beta) of the last build under
                                * msl_set_projection(R, J), species-major, then m = -R J .. (R+1) J - 1; MSL_BUF_FORMFACTOR is then empty */
    MSL_BUF_IONIZATION_WEIGHT = 18 /* (n,nz,nx,ny) f32  the ionisation weights W_e,s of the last build with msl_set_ionization */
} msl_buffer;

typedef struct {
    uint64_t slice_steps;      /* probes x slices propagated since create/reset             */
    uint64_t frames;           /* frames propagated                                         */
    uint64_t algorithmic_bytes;/* 16 B x nx x ny per slice-step on the one-pass loop, 32 B on the two-pass loop (+ t and epilogue terms) */
    double   ms_potential;     /* device time (HIP events) spent in potential builds        */
    double   ms_propagate;     /* ... in slice loops (+ epilogue)                           */
    double   ms_tacaw;
    uint64_t slice_kernel_launches; /* launches of the dominant slice-loop kernels         */
    double   ms_slice_kernels; /* device time of those launches only (HIP events on the handle's stream) */
    uint64_t row_launches;     /* row-pass launches (ifft_y, x t, fft_y, x Py) and their device time */
    double   ms_row;
    uint64_t col_launches;     /* column-pass launches (fft_x, x Px, ifft_x) and their device time   */
    double   ms_col;
} msl_counters;

int  msl_abi_version(void);
/* Which slice-loop kernel a line of n points gets (the reference's grids are int(L / sampling) + 1 points, potentials.py:123-125,
 * so a user picks the line lengths with `sampling`): 2 = power-of-two register kernel (256, 512, 1024, 2048), 1 = direct
 * mixed-radix pass (99 lengths 135 ... 1728 with factors 2, 3, 5, 7), 0 = any other length: zero-padded convolution on the next
 * power-of-two transform (2-4 x the work per point) or the generic LDS kernel.  No handle, no device needed. */
int  msl_line_kernel_class(int32_t n);
/* Message of the last failure on this handle (or of the last failed msl_create when h==NULL). */
const char* msl_last_error(const msl_handle* h);

/* Create / destroy.  Replaces the allocation side of MultisliceCalculator.setup()
 * (calculators.py:154-161: base probe, wavefunction_data zeros). */
int  msl_create(const msl_config* cfg, msl_handle** out);
int  msl_destroy(msl_handle* h);

/* Kirkland parameter table, 103 elements x 3 terms x (a,b,c,d), row-major doubles.
 * Replaces loadKirkland() (potentials.py:134-185). */
int  msl_set_kirkland(msl_handle* h, const double* abcd_103x3x4);

/* Slice bin edges [lo[s], hi[s]) along the beam axis, nz doubles each.
 * Replaces the slice_min/slice_max rule of Potential.__init__ (potentials.py:302-307). */
int  msl_set_slices(msl_handle* h, const double* lo, const double* hi);

/* Change the beam after create: recomputes the Fresnel tables and, when a potential V is held
 * (keep_potential), re-derives exp(i sigma V).  Lets Potential() (which knows no beam energy,
 * potentials.py:188) be built first and Propagate() (multislice.py:258-275) supply the beam. */
int  msl_set_beam(msl_handle* h, double wavelength, double sigma, double dz);

/* Specimen tilt: the beam is inclined to the slice normal by (theta_x, theta_y), small-angle -- the specimen is
 * sheared, not rotated -- so that free propagation through one slice moves the wave by (+dz tan_x, +dz tan_y), cyclically:
 *     P(kx, ky) = exp(-i pi lambda dz kx^2) exp(-2 pi i dz kx tan_x)  x  exp(-i pi lambda dz ky^2) exp(-2 pi i dz ky tan_y).
 * The pattern stays centred on the optic axis.  msl_set_tilt rewrites every propagator table of both axes (the plain tables, the
 * split-order copy, the layer tap's conjugates, the filters of the convolution kinds) with kernels on the handle's stream: phases in
 * float64, one rounding to float, no host table, no copy and no wait, so that a change of tilt is ordered behind the slice loops
 * queued before it.  Valid any time after msl_create; the tilt stays on the handle, and a later msl_set_beam rebuilds the tables
 * with it.  (0, 0) writes the untilted tables through the same kernels (equal to the host's up to one float rounding per entry);
 * a handle on which msl_set_tilt was never called keeps the host tables and runs bit for bit as before.  A built S-matrix
 * (msl_smatrix_build) belongs to the tilt it was built at and must be built again.  MSL_ERR_INVALID for a non-finite tangent; the
 * small-angle limit (200 mrad in pyslice_amd/tilt.py) is the caller's.
 * The one-pass kernels of a zero-padded convolution axis (msl_line_kernel_class 0, or a register length whose other axis is no
 * multiple of 16) and the 2048-point wave kernel keep one half of an even table and mirror the other, which a tilted axis does not
 * have.  While a non-zero tangent lies along such an axis the handle runs the two-pass loop (the loop of fft_path = 1 along that
 * axis, on the plain tables) and builds its potentials in natural order; the stacks already built are carried over on the stream.
 * That loop costs two launches per slice and the generic transform: lengths with a direct kernel (four-step, 2 R^2, mixed radix)
 * next to a multiple of 16 keep the one-pass loop under any tilt.  A zero tangent along the axis brings the one-pass loop back.
 * msl_get_tilt: tan_xy[0..1] = the tangents of the last msl_set_tilt, (0, 0) before the first.
 * Not in the reference, whose propagator (multislice.py:262-275) has no tilt. */
int  msl_set_tilt(msl_handle* h, double tan_x, double tan_y);
int  msl_get_tilt(const msl_handle* h, double* tan_xy);

/* Band limit (anti-aliasing): keep the signed FFT frequency indices |h_x| <= cut_x, |h_y| <= cut_y -- a
 * rectangle M(kx, ky) = m_x(kx) m_y(ky), separable and even -- in BOTH factors of every product t_k psi:
 *   - every propagator table of both axes is masked on the device (propagator_bandlimit_kernel, after the tables of msl_set_beam /
 *     msl_set_tilt are written and before the filters of the convolution kinds are summed): P -> P M, under any tilt;
 *   - every transmission stack is low-passed after its build, t_k -> ifft2(M fft2(t_k)), on the handle's stream with no host copy:
 *     msl_build_potential, msl_build_potentials, msl_build_thermal, msl_build_modes, msl_upload_potential, the absorptive build, and
 *     the stacks msl_set_beam re-derives.  MSL_BUF_TRANSMISSION downloads the limited stack, MSL_BUF_POTENTIAL stays the unlimited V.
 * With 3 cut_d < n_d the run is alias-free per axis: wave and t_k live in |h| <= cut, their product in |h| <= 2 cut, its fold-back at
 * |h| >= n - 2 cut > cut, which the next propagator zeroes.  The incident wave is not masked (the first propagator removes its
 * out-of-band part), and neither is the exit wave: the last operation of the slice loop is a transmission, so the exit spectrum is the
 * alias-free band |h| <= cut plus the product terms beyond it.  pyslice_amd/bandlimit.py is the definition and turns a fraction of
 * Nyquist into the cuts; integers here keep host and device from disagreeing on a bin at the edge.
 * Both cuts negative clear the limit: the tables of a handle without the call (the host tables when no tilt was ever set) and the
 * build path of today, bit for bit; clearing a handle that has no limit does nothing.  MSL_ERR_INVALID: one cut negative and the other
 * not, a cut below 1, 3 cut_d >= n_d.  Valid any time after msl_create; the limit stays on the handle.
 * Every effective call invalidates a built S-matrix (as msl_set_tilt does) and the resident potential: with a kept V (keep_potential,
 * no absorption; such a handle has one stack, frame_batch is ignored) the transmission functions are made again from it under the new limit, otherwise the potential is dropped
 * (msl_propagate is MSL_ERR_STATE until the next build).  The layer tap (msl_set_layers) inverts the propagator with its conjugate,
 * which a masked table does not have: the caller keeps the two apart (pyslice_amd refuses the combination).
 * msl_get_bandlimit: cut_xy[0..1] = the cuts, (-1, -1) without a limit.  Not in the reference, which has no band limit (quirk Q8). */
int  msl_set_bandlimit(msl_handle* h, int32_t cut_x, int32_t cut_y);
int  msl_get_bandlimit(const msl_handle* h, int32_t* cut_xy);

/* Re-size the probe batch (re-allocates the (P,nx,ny) working buffers; probes must be set again). */
int  msl_resize_probes(msl_handle* h, int32_t n_probes);

/* Build the P shifted probes on the device: psi0[p] = ifft2(mask * exp(2 pi i (kx px + ky py)) * centre-shift).
 * mrad == 0 gives plane waves (ones).  xy = P x 2 doubles (Angstrom).
 * Replaces Probe.__init__ + create_batched_probes (multislice.py:112-124, 198-235). */
int  msl_set_probes(msl_handle* h, double mrad, const double* xy, int32_t n_probes);

/* Aberration function of the probe-forming lens: every later msl_set_probes builds
 *     psi0[p] = ifft2(mask * ramp_p * exp(-i chi(k))),
 *     chi(k) = (2 pi / lambda) sum_nm C_nm / (n+1) * alpha^(n+1) * cos(m (phi - phi_nm)),  alpha = lambda |k|, phi = atan2(ky, kx).
 * polar = n_terms x 2 doubles (magnitude C_nm in Angstrom, angle phi_nm in radians; the angle is ignored for m == 0) in the order
 *     C10 C12 C21 C23 C30 C32 C34 C41 C43 C45 C50 C52 C54 C56.
 * n_terms must be 14, or 0 to clear (polar is then not read and may be NULL).  Non-finite values are MSL_ERR_INVALID.  C10 = +dz is the
 * reference's Probe.defocus(dz) for dz > 0 (exp(-i pi lambda dz k^2), multislice.py:183-190); a negative C10 is the conjugate
 * phase.  The state stays on the handle until it is set again or cleared, and uses the wavelength the handle has when
 * msl_set_probes runs.  All magnitudes zero is the same as cleared: msl_set_probes then runs exactly as without this call.
 * Plane waves (mrad == 0) have chi(0) = 0 and are not changed.  msl_upload_probes and msl_shift_probes, whose arrays come from
 * the caller, ignore the aberrations. */
int  msl_set_aberrations(msl_handle* h, const double* polar, int32_t n_terms);

/* Member probes of a partially coherent scan (pyslice_amd/coherence.py): msl_set_probes with a defocus of its own for every probe,
 *     psi0[p] = ifft2(mask * ramp_p * exp(-i chi_p(k))),   chi_p = the handle's chi with C10 + defocus[p]
 * (defocus = n_probes doubles in Angstrom, in the sense of C10: +dz is the reference's Probe.defocus(dz)); every other term comes from
 * msl_set_aberrations.  Same aperture rule, ramp and float64 polynomial of chi / (2 pi) in turns, reduced to one turn before the fp32
 * sincos.  MSL_ERR_INVALID for mrad == 0 (plane waves have no defocus), a non-finite defocus and what msl_set_probes refuses.  With
 * every defocus[p] == 0 the call IS msl_set_probes(h, mrad, xy, n_probes), bit for bit. */
int  msl_set_probe_members(msl_handle* h, double mrad, const double* xy, const double* defocus, int32_t n_probes);

/* Upload arbitrary initial waves (P,nx,ny) c64 (used when a caller hands Propagate() a
 * Probe built from its own array, multislice.py:104-109). */
int  msl_upload_probes(msl_handle* h, const float* c64, int32_t n_probes);

/* Shift an arbitrary base probe (nx,ny) c64 to P positions: psi0[p] = ifft2(fft2(base) * ramp_p).
 * Replaces create_batched_probes for probes built from a caller array (multislice.py:216-227). */
int  msl_shift_probes(msl_handle* h, const float* base_c64, const double* xy, int32_t n_probes);

/* Execution model: one handle = one HIP device + one stream.  With msl_config.launch_timing == 0 the per-frame calls
 * (msl_build_potential, msl_propagate, msl_propagate_frame) copy their host arguments into library-owned pinned memory,
 * queue the work on the stream and return; results are complete after msl_synchronize or any msl_download* call (which
 * wait for the stream).  With launch_timing == 1 they also wait, so that msl_get_counters can attribute time. */

/* Projected Kirkland potential + transmission functions of one MD frame.
 * pos = n x 3 doubles, Z = n atomic numbers (1..103); ax1/ax2 = in-plane axes, axs = slice axis.
 * Replaces Potential.__init__ (potentials.py:188-348) and the per-slice exp(i sigma V) of
 * Propagate (multislice.py:281-282). */
int  msl_build_potential(msl_handle* h, const double* pos, const int32_t* Z, int64_t n_atoms,
                         int32_t ax1, int32_t ax2, int32_t axs);

/* Upload a caller-made potential V (nz,nx,ny) float32 slice-major and derive exp(i sigma V)
 * (Propagate() accepts any Potential object, multislice.py:237). */
int  msl_upload_potential(msl_handle* h, const float* V_nz_nx_ny);

/* Slice loop for all probes against the current potential: nz transmissions, nz-1 Fresnel steps.
 * Leaves real-space exit waves in MSL_BUF_EXIT.  Replaces Propagate() (multislice.py:237-299). */
int  msl_propagate(msl_handle* h);

/* Slice loop + fused epilogue fftshift(fft2(exit)) written into frame slot `slot` of the
 * (P,T_local,nx,ny) result.  Replaces _process_frame_worker_torch after the potential
 * (calculators.py:281-290) and the scatter loop (calculators.py:185-186). */
int  msl_propagate_frame(msl_handle* h, int32_t slot);

/* Frame batching (msl_config.frame_batch = B > 1).  msl_select_batch_slot picks the transmission stack (0 <= b < B) that the
 * next msl_build_potential / msl_upload_potential fills and that msl_propagate / msl_propagate_frame use;
 * msl_propagate_frames runs the slice loop + exit FFT for the frames in batch slots 0..count-1 in ONE sequence of
 * launches and writes them to frame slots first_slot .. first_slot+count-1 of the (P,T_local,wx,wy) result.
 * msl_frame_batch returns the batch size the handle really uses (1 when batching is off).
 * Replaces count iterations of the reference's serial frame loop (calculators.py:172-186). */
int  msl_select_batch_slot(msl_handle* h, int32_t b);
int  msl_propagate_frames(msl_handle* h, int32_t first_slot, int32_t count);
/* The potentials of `count` MD frames (1 <= count <= frame_batch) into the batch slots 0 .. count-1 in ONE sequence of launches:
 * pos = count x n_atoms x 3 doubles (frame-major), Z = the n_atoms atomic numbers every frame shares (Trajectory.atom_types,
 * trajectory.py:8-14); axes as msl_build_potential.  Replaces `count` constructions of Potential (calculators.py:172-186 builds
 * one per frame, potentials.py:188-348) -- with the reference's default single probe the per-frame build is the frame. */
int  msl_build_potentials(msl_handle* h, const double* pos, const int32_t* Z, int64_t n_atoms, int32_t count,
                          int32_t ax1, int32_t ax2, int32_t axs);
int  msl_frame_batch(const msl_handle* h);

/* ---- frozen phonons: Einstein-model configurations generated on the device ----
 * A configuration is a pure function of (seed, configuration index c, atom index i) -- pyslice_amd/thermal.py is the definition:
 *   x0..x3 = Philox-4x32-10(counter (i, c & 0xffffffff, c >> 32, 0), key (seed & 0xffffffff, seed >> 32)),  u_j = (x_j + 0.5) 2^-32,
 *   pos = pos0 + sigma_i * (sqrt(-2 ln u0) cos(2 pi u1), sqrt(-2 ln u0) sin(2 pi u1), sqrt(-2 ln u2) cos(2 pi u3))
 * in columns 0, 1, 2 of the positions whatever the axes are, in float64, not wrapped and not clipped: the slice rule of
 * msl_build_potential treats the result as it treats an MD frame (an atom pushed out of the stack is dropped).
 * msl_set_structure:  uploads ONCE the base positions pos0 (n_atoms x 3 doubles), the atomic numbers Z (1..103), the rms displacement
 *   sigma per atom and Cartesian axis (Angstrom, finite and >= 0) and the species maps; they stay resident on the handle until the
 *   next msl_set_structure or msl_destroy.  Axes as msl_build_potential.  MSL_ERR_INVALID names a bad Z or sigma.  Synchronous: no
 *   pointer into caller memory is kept.
 * msl_build_thermal:  the potentials and transmission functions of the configurations first_config .. first_config + count - 1
 *   (1 <= count <= frame_batch, first_config >= 0) into the batch slots 0 .. count-1, as msl_build_potentials fed those positions; at
 *   a frame batch of 1 into the selected slot, as msl_build_potential.  The same sequence of launches with one stage exchanged:
 *   thermal_positions_kernel writes the positions where msl_build_potentials copies them to, so nothing per frame crosses PCIe or
 *   is staged on the host, and the result is bit for bit that of msl_build_potentials given msl_thermal_positions' arrays.
 *   MSL_ERR_INVALID without msl_set_structure.  Queued on the stream like msl_build_potential.
 * msl_thermal_positions: the positions the device generates for one configuration, n_atoms x 3 doubles, downloaded (waits for the
 *   stream).
 * Not built: anisotropic or per-axis widths, wrapping at the entrance and exit surfaces.  Correlated (phonon-mode) displacements:
 * msl_set_modes, below.
 * Not in the reference, whose Trajectory.generate_random_displacements (trajectory.py:226) fabricates uniform noise on the host. */
int  msl_set_structure(msl_handle* h, const double* pos0, const int32_t* Z, const double* sigma, int64_t n_atoms,
                       int32_t ax1, int32_t ax2, int32_t axs);
int  msl_build_thermal(msl_handle* h, uint64_t seed, int64_t first_config, int32_t count);
int  msl_thermal_positions(msl_handle* h, uint64_t seed, int64_t config, double* out);

/* ---- phonon modes: lattice-dynamics frames synthesised on the device ----
 * A frame is a pure function of (seed, frame index c) -- pyslice_amd/phonons.py is the definition.  M modes, each with a wave vector
 * q_m (Cartesian, cycles / Angstrom, columns 0, 1, 2 like the positions whatever the axes are), a phase advance tau_m (cycles per
 * frame) and a complex displacement W[m, b, :] (Angstrom) of every basis atom b; atom i is basis atom b_i at the base position r_i:
 *   g_m(k) = sqrt(-ln u0) exp(2 pi i u1),  u from Philox-4x32-10(counter (m, k & 0xffffffff, k >> 32, 1), key as msl_build_thermal)
 *   dynamic: k = 0, theta = tau_m c (a time-coherent record)      else: k = c, theta = 0 (independent snapshots)
 *   C[c,m] = g_m(k) exp(-2 pi i frac(theta)),  E = exp(2 pi i frac((q0 r0 + q1 r1) + q2 r2)),  frac(y) = y - rint(y)
 *   pos = r_i + sum_m Re[(C[c,m] E) W[m, b_i, :]]      in float64, summed in mode order, not wrapped and not clipped
 * msl_set_modes:  requires msl_set_structure (whose sigma the mode builds ignore); uploads ONCE basis_index (n_atoms int32 in
 *   [0, n_basis)), q (n_modes x 3 doubles), tau (n_modes doubles, finite and >= 0), W (n_modes x n_basis x 3 complex doubles, re/im
 *   interleaved) and the frame rule; they stay resident until the next msl_set_modes, msl_set_structure (which drops them) or
 *   msl_destroy.  n_atoms is the length of basis_index and must be the structure's atom count.  MSL_ERR_INVALID names what was
 *   wrong: a bad index, a non-finite value, a negative tau, n_modes < 1, n_basis < 1, an atom count that disagrees with the
 *   structure.  A refused call leaves the resident modes as they were.  Synchronous: no pointer into caller memory is kept.
 * msl_build_modes:  the mirror of msl_build_thermal -- the potentials and transmission functions of the frames first_frame ..
 *   first_frame + count - 1 (1 <= count <= frame_batch, first_frame >= 0; first_frame + count <= 2^31 when dynamic) into the same
 *   batch slots, by the same sequence of launches with the position stage exchanged: mode_coefficients_kernel fills the (count, M)
 *   table C, mode_positions_kernel writes the positions where msl_build_potentials copies them to.  Bit for bit
 *   msl_build_potentials given msl_mode_positions' arrays.  MSL_ERR_INVALID without msl_set_modes.  Queued on the stream.
 * msl_mode_positions: the positions the device generates for one frame, n_atoms x 3 doubles, downloaded (waits for the stream).
 * Not built: Einstein widths on top of the modes, anharmonic or damped modes, occupations that change over time, fp32 or
 * table-driven phases.  Not in the reference. */
int  msl_set_modes(msl_handle* h, const int32_t* basis_index, int64_t n_atoms, int32_t n_basis, const double* q, const double* tau,
                   const double* W, int32_t n_modes, int32_t dynamic);
int  msl_build_modes(msl_handle* h, uint64_t seed, int64_t first_frame, int32_t count);
int  msl_mode_positions(msl_handle* h, uint64_t seed, int64_t frame, double* out);

/* ---- absorptive potential: Debye-Waller damping and TDS absorption in one pass ----
 * The thermal average of the elastic wave without an ensemble: every later msl_build_potential / msl_build_potentials makes
 *     t_s = exp(i sigma Vbar_s - sigma^2 Omega_s)
 * Vbar the Debye-Waller-smeared mean potential, Omega = 1/2 Var V under independent Gaussian displacements (the second cumulant of
 * <exp(i sigma V)>; pyslice_amd/absorptive.py is the definition).  Per species, on the handle's grid, with D = exp(-2 pi^2 u^2 q^2):
 *     Vbar1 = Re ifft2(f D) / (dx^2 dy^2),  Om1 = 1/2 (Re ifft2(D fft2(V1^2)) - Vbar1^2),  g = Re fft2(Om1) dx^2 dy^2
 * and Vbar, Omega are the structure-factor sums of the potential build with the tables f D and g.
 * u_by_Z_103: the rms displacement per Cartesian axis (Angstrom, finite and >= 0) of every atomic number 1..103 -- the sigma of
 *   msl_set_structure; NULL clears absorption and frees its tables and stacks: the next build is that of a handle it was never set on.
 * absorb == 0 keeps the Debye-Waller damping and leaves Omega out (|t| = 1).
 * Every call drops the potential the handle holds (msl_propagate is MSL_ERR_STATE until the next build): the transmission functions
 *   and the stacks of an earlier build belong to the widths and the flag they were built with.
 * While it is set: MSL_BUF_FORMFACTOR is f D, MSL_BUF_FORMFACTOR_ABS g, MSL_BUF_POTENTIAL Vbar (also without keep_potential),
 * MSL_BUF_ABSORPTION Omega, each of the current batch slot; msl_set_beam makes t again from the two resident stacks (Omega and g do not
 * depend on sigma); msl_build_thermal / msl_build_modes return MSL_ERR_STATE -- the vibration would be counted twice.  Costs two
 * float32 stacks (frame_batch, nz, nx, ny) and a second structure factor and inverse transform per build.  The model is the classical
 * weak-fluctuation one: third order in sigma V per atom.  Synchronous.  Not in the reference. */
int  msl_set_absorption(msl_handle* h, const double* u_by_Z_103, int32_t absorb);

/* ---- TDS detector signal of the absorptive potential: HAADF from one pass ----
 * What the absorption takes out of the elastic wave in slice s and detector d collects, in the local approximation (pyslice_amd/tds.py
 * is the definition):
 *     I[p, d, s] = sum_r |psi_p,s(r)|^2 w_d,s(r),   w_d,s = 1 - exp(-2 sigma^2 Omega_det,d,s),   psi_p,s = the wave arriving at slice s
 * Omega_det the structure-factor sum with the detector-restricted tables g_det: per species, M_d the membership,
 *     V1M = Re ifft2(M f) / (dx^2 dy^2),  Vbar1M = Re ifft2(M f D) / (dx^2 dy^2),
 *     Om1det = 1/2 (Re ifft2(D fft2(V1 V1M)) - Vbar1 Vbar1M),  g_det = Re fft2(Om1det) dx^2 dy^2
 * (M = 1: Om1 and g).  TDS electrons are not propagated further.
 * msl_set_tds:  member_bits = (nx, ny) uint16 on the fftfreq grid, unshifted, bit d = detector d, 1 <= n_det <= 4; NULL or n_det = 0
 *   clears it and frees its buffers.  MSL_ERR_STATE without msl_set_absorption(.., absorb != 0) (clearing or changing that to
 *   absorb == 0 clears this too); MSL_ERR_UNSUPPORTED at a frame batch above 1.  Drops the potential as msl_set_absorption does: the
 *   next build makes g_det (MSL_BUF_FORMFACTOR_TDS) and, per detector, one more structure factor and inverse transform into the
 *   weight stack (MSL_BUF_TDS_WEIGHT), which msl_set_beam remakes for another sigma.  While it is set every msl_propagate* runs
 *   the two-pass loop with the row step of each slice in two launches and the reduction between them: about 3.5 times the
 *   one-pass loop's bytes.  The exit waves and spectra are those of the two-pass loop, bit for bit.  Synchronous.
 * msl_tds_fetch:  after one stream synchronisation, I of the last slice loop for the first B probes (B <= 0: n_probes) as
 *   (nz, B, n_det) float64 on the host.  MSL_ERR_STATE before the first loop.
 * msl_tds_reduce:  the reduction alone, of the work buffer as the last slice loop left it (MSL_BUF_EXIT) against the weights of
 *   `slice`: the tile kernel `reps` times between two events and the finishing sum once.  out (n_probes, n_det) float64 and
 *   ms_reduce, the mean device time of one repeat in ms, may be NULL.  For benchmarks.  Not in the reference. */
int  msl_set_tds(msl_handle* h, const uint16_t* member_bits, int32_t n_det);
int  msl_tds_fetch(msl_handle* h, int32_t B, double* out);
int  msl_tds_reduce(msl_handle* h, int32_t slice, int32_t reps, double* out, double* ms_reduce);

/* ---- element maps: channelling-weighted ionisation signal per element ----
 * What an EDX or core-loss EELS map records, in the local approximation (pyslice_amd/ionization.py is the definition): per channel e
 * -- an atomic number Z_e, a Gaussian of rms width w_e (Angstrom) and a cross-section c_e (Angstrom^2) -- and slice s, with A_e,s
 * the atoms of that element the build puts into slice s (its own slice rule),
 *     W_e,s(r) = Re ifft2( c_e exp(-2 pi^2 w_e^2 |k|^2) sum_{i in A_e,s} exp(-2 pi i k r_i) ) / (dx dy)      (sum_r W dx dy = c_e |A_e,s|)
 *     I[p, e, s] = sum_r |psi_p,s(r)|^2 W_e,s(r) / sum_r |psi_p,0(r)|^2,       psi_p,s = the wave arriving at slice s
 * the ionisation probability per incident electron in slice s.  The elastic wave is not depleted and the ionised electrons are not
 * followed.
 * msl_set_ionization:  1 <= n <= 8 channels (two may name one element); n = 0 or a NULL array clears it and frees its buffers.
 *   Independent of msl_set_absorption.  MSL_ERR_INVALID: n > 8, an atomic number outside 1..103, a width that is not finite and
 *   positive, a cross-section that is not finite and >= 0.  MSL_ERR_UNSUPPORTED at a frame batch above 1 and under
 *   msl_set_projection (which is MSL_ERR_UNSUPPORTED while this is set).  MSL_ERR_STATE while msl_set_tds is set (and msl_set_tds is
 *   MSL_ERR_STATE while this is set): a handle runs one per-slice reduction.  Drops the potential as msl_set_tds does: the next
 *   build (msl_build_potential, msl_build_thermal, msl_build_modes) makes, per channel, a table that is non-zero for its species
 *   only and with it one more structure factor and inverse transform of the positions it has just placed, into the weight stack
 *   (MSL_BUF_IONIZATION_WEIGHT); a channel whose element the structure does not hold gives zeros.  While it is set every
 *   msl_propagate* runs the two-pass loop with the row step of each slice in two launches and the reduction between them, as under
 *   msl_set_tds; the exit waves and spectra are those of the two-pass loop, bit for bit.  Synchronous.
 * msl_ionization_fetch:  after one stream synchronisation, I of the last slice loop for the first B probes (B <= 0: n_probes) as
 *   (nz, B, n) float64 on the host.  MSL_ERR_STATE before the first loop.
 * msl_ionization_reduce:  the reduction alone, of the work buffer as the last slice loop left it (MSL_BUF_EXIT) against the weights
 *   of `slice`: the tile kernel `reps` times between two events and the finishing sum once.  out (n_probes, n) float64 -- the sums
 *   sum_r |psi|^2 W, not divided by a norm -- and ms_reduce, the mean device time of one repeat in ms, may be NULL.  For benchmarks.
 *   Not in the reference. */
int  msl_set_ionization(msl_handle* h, int32_t n, const int32_t* Z, const double* width, const double* cross_section);
int  msl_ionization_fetch(msl_handle* h, int32_t B, double* out);
int  msl_ionization_reduce(msl_handle* h, int32_t slice, int32_t reps, double* out, double* ms_reduce);

/* ---- gradients: the slice loop backwards ----
 * The derivative of a data-fit loss of the exit patterns I = |Psi|^2, Psi = fft2(t_nz-1 psi_nz-1), against measured patterns D with
 * respect to the slice potentials (pyslice_amd/adjoint.py is the definition).  With G = dL/dPsi* (dL = 2 Re sum conj(G) dPsi) and an
 * optional detector weight w >= 0:
 *     MSL_ADJ_AMPLITUDE  L = sum w (sqrt I - sqrt D)^2          G = w (1 - sqrt D / max(|Psi|, sqrt eps)) Psi
 *     MSL_ADJ_INTENSITY  L = 1/2 sum w (I - D)^2                G = w (I - D) Psi
 *     MSL_ADJ_POISSON    L = sum w (I - D log(I + eps))         G = w (1 - D / (I + eps)) Psi
 * Backwards: g = nx ny ifft2(G); for s = nz - 1 .. 0: dL/dV_s += 2 sigma sum_p Im(g_p conj(t_s psi_p,s)), g <- conj(t_s) g, and for
 * s > 0 g <- ifft2(conj(P) fft2 g) with the handle's own propagator tables (a tilt is carried).  After s = 0, g is dL/dpsi_0*.
 * msl_set_adjoint:  loss_kind = MSL_ADJ_OFF switches it off and frees its buffers.  Else allocates the wave stack (nz - 1, n_probes,
 *   nx, pitch) c64 (psi_0 is the probe buffer), the float64 accumulator (nz, nx, ny), zeroed, and the data of one probe batch, and
 *   puts the handle on the two-pass loop; weight: (nx, ny) f32 in the layout of D, or NULL.  MSL_ERR_UNSUPPORTED under a band limit,
 *   an absorptive potential, a frame batch above 1, layers or a layer reduction; MSL_ERR_STATE under msl_set_tds / msl_set_ionization
 *   (which are MSL_ERR_STATE while this is set); MSL_ERR_NOMEM names the bytes wanted: a handle of fewer probes makes the stack fit.
 *   While it is set msl_propagate* run the plain two-pass loop.  Synchronous.
 * msl_adjoint_reset:  zeroes the accumulator (queued).
 * msl_adjoint_add:  for the handle's probes and potential: the forward loop, which keeps psi_s between the two launches of every row
 *   step, the exit FFT, the residual against data (B, nx, ny) f32 on the host -- the fftshifted layout and the units of msl_diffract
 *   at bin 1 without a k-window -- and the backward loop, added into the accumulator.  Takes the first B <= n_probes probes;
 *   loss_out (B) float64; probe_grad (B, nx, ny) c64 or NULL.  No atomics: the same calls give the same bits.  The work buffer ends
 *   as the probe gradient (MSL_BUF_EXIT is stale).  Synchronous.
 * msl_adjoint_download:  the accumulator, (nz, nx, ny) float64.  Synchronous.
 * msl_adjoint_step_time:  the step kernel of `slice` alone over the n_probes images of the work buffer as the last call left it, once
 *   untimed and then `reps` times between two events; ms_step = the mean device time of one launch in ms.  It adds into row `slice`
 *   of the accumulator and rewrites the work buffer: msl_adjoint_reset afterwards.  For benchmarks, as msl_tds_reduce is.
 * msl_adjoint_layout:  read-only, for tests: *pitch = the row pitch of the work buffer and the wave stack in elements, *vec = 1 where
 *   msl_adjoint_add launches the 16-byte variant of the step kernel (an even pitch, buffers on 16 bytes), 0 for the 8-byte one.  Either
 *   pointer may be NULL.  MSL_ERR_STATE without msl_set_adjoint (no message is set: the handle is const).
 * Not in the reference. */
enum { MSL_ADJ_OFF = 0, MSL_ADJ_AMPLITUDE = 1, MSL_ADJ_INTENSITY = 2, MSL_ADJ_POISSON = 3 };
int  msl_set_adjoint(msl_handle* h, int32_t loss_kind, double epsilon, const float* weight);
int  msl_adjoint_reset(msl_handle* h);
int  msl_adjoint_add(msl_handle* h, const float* data, int32_t B, double* loss_out, void* probe_grad);
int  msl_adjoint_download(msl_handle* h, double* grad);
int  msl_adjoint_step_time(msl_handle* h, int32_t slice, int32_t reps, double* ms_step);
int  msl_adjoint_layout(const msl_handle* h, int32_t* pitch, int32_t* vec);

/* ---- gradients with respect to atom positions: the potential build backwards ----
 * The build is V_s = Re ifft2( sum_Z f_Z sum_{a in Z, s} e^{-2 pi i (kx x_a + ky y_a)} ) / (dx^2 dy^2) on the fftfreq grid.  With
 * Gamma_s = dL/dV_s, B_s = fft2(Gamma_s) and c = 2 pi / (nx ny dx^2 dy^2), for atom a of species Z in slice s
 *     dL/dx_a = c sum_{kx, ky} kx f_Z(k) Im( conj(B_s(k)) e^{-2 pi i kx x_a} e^{-2 pi i ky y_a} ),     dL/dy_a: the same with ky,
 * over the full grid (pyslice_amd/adjoint.py: position_gradient is the definition).  The derivative along the slice axis is zero (an
 * atom is binned, not spread); an atom in no slice gets zeros.
 * msl_adjoint_positions:  gamma == NULL takes Gamma from the accumulator of msl_adjoint_add (MSL_ERR_STATE without msl_set_adjoint);
 *   else gamma is the caller's (nz, nx, ny) float64 dL/dV on the host, uploaded -- msl_set_adjoint is not needed then.  out: (n, 3)
 *   float64 on the host, in the order and the axes of the positions msl_build_potential was given: columns ax1 and ax2 hold the two
 *   components, column axs is zero.  Reads the sorted phase tables, the order, the bin starts and the form-factor tables that the
 *   last msl_build_potential left on the device: MSL_ERR_STATE, naming the missing build, when no single-frame build is resident --
 *   before the first build, and after msl_build_potentials of more than one frame, msl_build_thermal, msl_build_modes,
 *   msl_upload_potential, msl_set_projection, msl_set_absorption (and what drops the potential with them: msl_set_tds,
 *   msl_set_ionization), or a build under finite projection or absorption.  Gamma is rounded to float32, transformed by the handle's
 *   own 2-D FFT, and position_gradient_kernel gathers at the atoms in exact float32 products with float64 sums; no atomics: the same
 *   calls give the same bits.  Leaves the work buffer, the potential and the accumulator as they are.  Synchronous.
 *   A build under a band limit (msl_set_bandlimit) does not count either: its V is low-passed behind the structure factor.
 *   Device memory of its own, grown on demand and freed by msl_set_adjoint(MSL_ADJ_OFF) and msl_destroy: the images of a chunk of
 *   slices (at most 256 MB, or one image), an uploaded gamma (8 nz nx ny bytes), the tile list and the result.
 * msl_adjoint_positions_rows:  the rows n that msl_adjoint_positions would write now, or -1 where it would be MSL_ERR_STATE for want
 *   of a build: what a caller sizes `out` by.
 * msl_adjoint_positions_time:  the chain on the accumulator (conversion, transforms, kernel), once untimed and then `reps` times
 *   between two events; ms_chain = the mean device time of one chain in ms.  For benchmarks.
 * Not in the reference. */
int  msl_adjoint_positions(msl_handle* h, const double* gamma, double* out);
int64_t msl_adjoint_positions_rows(const msl_handle* h);
int  msl_adjoint_positions_time(msl_handle* h, int32_t reps, double* ms_chain);

/* ---- gradients with respect to scan positions and probe aberrations: the probe recipe backwards ----
 * msl_set_probes builds psi0_p = ifft2(Phi_p), Phi_p(k) = A(k) exp(2 pi i (t_ramp,p(k) - chi(k) / 2 pi)): the strict aperture |k| < radius,
 * t_ramp,p = fx (floor(nx/2)/nx + x_p/Lx) + fy (floor(ny/2)/ny + y_p/Ly) on signed frequency indices, and chi / 2 pi = sum_j (a_j A_j(k) +
 * b_j B_j(k)) in the Cartesian form of msl_set_aberrations' fourteen terms.  With g0 = dL/dpsi0_p*, ghat = fft2(g0) (unnormalised),
 * N = nx ny and m_p(k) = Im(conj(ghat(k)) Phi_p(k)),
 *     dL/dx_p = -(4 pi / N) sum_k kx m_p(k),     dL/da_j = +(4 pi / N) sum_k A_j(k) m_p(k)     (ky, B_j likewise)
 * (pyslice_amd/adjoint.py: probe_parameter_gradient is the definition).
 * msl_adjoint_probe_params:  out: (B, 30) float64 on the host; per probe dL/dx, dL/dy (per Angstrom), then fourteen pairs (dL/da_j,
 *   dL/db_j) of that probe's share, b of the three m = 0 terms zero -- the lens is shared, so the derivative of the total loss is the
 *   sum over the probes.  g0 == NULL takes the probe gradient that the last msl_adjoint_add left in the work buffer (MSL_ERR_STATE
 *   without one of at least B images); else g0 is the caller's (B, nx, ny) c64 on the host, uploaded into the work buffer at its
 *   pitch -- msl_set_adjoint is not needed then.  Runs the handle's own 2-D FFT on the work buffer and probe_moment_kernel over the
 *   aperture's bounding box, float64 sums, no atomics: the same calls give the same bits.  The work buffer ends as the transforms
 *   (MSL_BUF_EXIT is stale, and so is the probe gradient).  Synchronous.
 *   Only probes built by msl_set_probes with mrad > 0 have a recipe: MSL_ERR_STATE, naming the missing call, after
 *   msl_upload_probes, msl_shift_probes, msl_set_probe_members, msl_smatrix_build / msl_smatrix_probes, msl_resize_probes, a later
 *   msl_set_aberrations or a changed wavelength (msl_set_beam) until the next msl_set_probes, and for plane waves.  The kernel reads
 *   the coefficients, the wavelength and the positions that msl_set_probes used, kept with the flag.  B outside [1, n_probes] or a
 *   NULL out: MSL_ERR_INVALID.
 * msl_adjoint_probe_params_time:  the chain (transform, kernel, sums) on the n_probes images of the work buffer as it stands, once
 *   untimed and then `reps` times between two events; ms_chain = the mean device time of one chain in ms.  For benchmarks.
 * Not in the reference. */
int  msl_adjoint_probe_params(msl_handle* h, const void* g0_c64_or_null, int32_t B, double* out);
int  msl_adjoint_probe_params_time(msl_handle* h, int32_t reps, double* ms_chain);

/* TACAW: intensity[p,w,kx,ky] = | fftshift_t fft_t( Psi - <Psi>_t ) |^2 over a (B,T,npix) c64 device
 * array.  src == NULL uses the handle's own wavefunction buffer (B=P, T=T_local, npix=nx*ny) and
 * its own intensity buffer.  With src/dst given (device pointers, e.g. the output of an RCCL
 * all-to-all held by the caller) the transform is applied to that memory.
 * Replaces TACAWData.fft_from_wf_data (tacaw_data.py:89-104). */
int  msl_tacaw(msl_handle* h, const void* d_src_c64, void* d_dst_f32, int64_t batch, int32_t T, int64_t npix);

/* Windowed, segment-averaged (Welch) TACAW spectra.  For every pixel's time line x[0..T), with segment length L, hop (1 <= hop <= L),
 * S = 1 + (T - L) / hop segments (frames past the last full segment are dropped) and a window w[0..L):
 *     r_s[n] = x[s hop + n] - x[s hop]
 *     y_s[n] = g[n] (r_s[n] - mean_n r_s[n]),      g = w sqrt(L / (S sum w^2))       (float64 here, a float32 table on the device)
 *     I[f]   = sum_s | sum_n y_s[n] exp(-2 pi i f n / L) |^2,      I[0] := 0 exactly
 * stored fftshifted along f: (batch, L, npix) float32; frequencies = fftshift(fftfreq(L, dt)).  L = T, hop = T and a boxcar window
 * give msl_tacaw's intensity; otherwise it is scipy.signal.welch(x, window=w, nperseg=L, noverlap=L-hop, detrend='constant',
 * return_onesided=False, scaling='density') * L outside f = 0.
 * Pointers as msl_tacaw: both NULL = the handle's own wavefunction buffer into its own intensity buffer, which then holds (P, L, pitch)
 * (the reductions with d_src == NULL see F = L).  window_L = L non-negative host doubles with sum w^2 > 0, NULL = boxcar.
 * MSL_ERR_INVALID for T < 2, L > T, hop outside [1, L], a negative, non-finite or all-zero window; MSL_ERR_UNSUPPORTED for an L
 * without a kernel (msl_tacaw_welch_has) or an image whose rows leave the kernel's 32-bit offsets ((L + 1) / 2 * npix * 8 >= 2^32).
 * One launch, no atomics: repeated calls are bitwise equal.  The counters take the device time (ms_tacaw) and the bytes the call
 * reads and writes, batch * npix * (8 S L + 4 L) (algorithmic_bytes).
 * msl_tacaw_welch_has: 1 if a kernel exists for segment length L (the 2-3-5-7-smooth lengths 16 ... 128), else 0.  No handle, no
 * device needed.
 * Not in the reference, whose transform is the bare periodogram (tacaw_data.py:89-104). */
int  msl_tacaw_welch_has(int32_t L);
int  msl_tacaw_welch(msl_handle* h, const void* d_src_c64, void* d_dst_f32, int64_t batch, int32_t T, int64_t npix,
                     int32_t L, int32_t hop, const double* window_L);

/* Streaming TACAW: the time -> frequency transform accumulated tile of frames by tile of frames, for n_bins
 * chosen frequency bins, so that the handle holds a ring of frame slots (msl_config.n_frames = tile length) and the
 * accumulators instead of every frame (the reference needs the whole (P,T,nx,ny) array: tacaw_data.py:94-96).
 *   begin:  T_total = frames of the run, bins = n_bins unshifted FFT bin numbers u in [0,T_total) (NULL: all T_total);
 *   push:   folds the frames in slots [first_slot, first_slot+count), whose time indices are t0, t0+1, ..;
 *   finish: intensity[p,i,k] = | sum_t Psi[p,t,k] exp(-2 pi i bins[i] t / T) |^2 (0 for bin 0: mean subtraction) becomes the
 *           handle's intensity buffer, shape (P, n_bins, K), ready for the reductions below; total_PK (host, P*K float64,
 *           may be NULL) receives sum over ALL T_total bins of the intensity (Parseval: T sum|Psi|^2 - |sum Psi|^2), i.e.
 *           TACAWData.diffraction() of the full transform without any of it being stored. */
int  msl_tacaw_stream_begin(msl_handle* h, int32_t T_total, int32_t n_bins, const int32_t* bins);
int  msl_tacaw_stream_push(msl_handle* h, int32_t first_slot, int32_t count, int32_t t0);
int  msl_tacaw_stream_finish(msl_handle* h, double* total_PK);
/* Reference pattern of an open stream: every frame pushed afterwards is folded as Psi[p,t,k] - ref[p,k].  A time-independent
 * offset only changes the u = 0 bin, which the reference's mean subtraction (tacaw_data.py:94) zeroes anyway, so the result is
 * unchanged -- but the float32 accumulators then hold the thermal part instead of T Bragg amplitudes that have to cancel.
 * d_ref_c64: device (P,K) c64, or NULL to take frame slot `slot` of this handle's ring.  Call it before the first push; all
 * handles that share one run (frame shards) must use the SAME reference (MSL_BUF_STREAM_REF gives the pointer to broadcast). */
int  msl_tacaw_stream_set_reference(msl_handle* h, const void* d_ref_c64, int32_t slot);
/* Frame-sharded runs (one handle per GPU, each pushing its own frames with their global time indices t0): the partial sums
 * MSL_BUF_STREAM_ACC / _S1 / _S2 are linear in the frames, so the caller sum-reduces them over the handles (RCCL
 * reduce-scatter over probes: pyslice_amd/distributed.py) into the probe range [p0, p0+count) of THIS handle's buffers and
 * then finishes that range only: intensity (count, n_bins, K) f32 into d_dst_f32 (device; NULL only for the full range, which
 * goes to the handle's intensity buffer like msl_tacaw_stream_finish), total_host (count*K f64, may be NULL).  Closes the stream.
 * Replaces, together with the pushes, TACAWData.fft_from_wf_data on the (P,T,nx,ny) array no rank holds (tacaw_data.py:89-104). */
int  msl_tacaw_stream_finish_range(msl_handle* h, int32_t p0, int32_t count, void* d_dst_f32, double* total_host);

/* ---- consumers of the resident results: reductions that stream the array once on the device ----
 * The TACAW reductions take a (B,F,K) float32 intensity array: d_src == NULL selects the handle's own intensity buffer
 * (B=P, F=T after msl_tacaw or n_bins after msl_tacaw_stream_finish, K=stored pixels); otherwise a caller-held device pointer with the given shape.  Results are
 * written to HOST memory; sums are accumulated in float64 like the reference's.
 * ld = distance in elements between consecutive (b,f) rows of K pixels (0: K; ignored with d_src == NULL): the library's own
 * result buffers keep every image at a pitch of msl_result_pitch() >= K pixels, so a pointer INTO them goes with that ld.
 *
 * msl_tacaw_spectrum: out[b*F+f] = sum_k w(k) I[b,f,k], w = 1 or mask[k] != 0 (mask: K host bytes or NULL).
 *   Replaces the k-space sums of TACAWData.spectrum (tacaw_data.py:109-143), spectrum_image (:145-179) and
 *   masked_spectrum (:256-300); the mean over probes / the frequency pick is a lookup in the (B,F) result. */
int  msl_tacaw_spectrum(msl_handle* h, const void* d_src_f32, int64_t B, int64_t F, int64_t K, int64_t ld, const uint8_t* mask, double* out);
/* msl_tacaw_spectrum_weighted: out[b*F+f] = sum_k weight[k] I[b,f,k] with K float64 host weights: a non-boolean mask of
 *   TACAWData.masked_spectrum, which multiplies the intensity (tacaw_data.py:286-296). */
int  msl_tacaw_spectrum_weighted(msl_handle* h, const void* d_src_f32, int64_t B, int64_t F, int64_t K, int64_t ld, const double* weight, double* out);
/* msl_tacaw_diffraction: out[k] = scale * sum_{b0<=b<b1} sum_{f0<=f<f1} I[b,f,k]   (K float64).
 *   Replaces TACAWData.diffraction (tacaw_data.py:183-217: all f, one probe or scale=1/P over all probes) and
 *   spectral_diffraction (:219-254: one f). */
int  msl_tacaw_diffraction(msl_handle* h, const void* d_src_f32, int64_t B, int64_t F, int64_t K, int64_t ld, int64_t b0, int64_t b1,
                           int64_t f0, int64_t f1, double scale, double* out);
/* msl_tacaw_dispersion: out[(b*F+f)*n + i] = I[b,f,idx[i]] for n flat k indices (kx*ny+ky) along a path (float32).
 *   Replaces the gather loop of TACAWData.dispersion (tacaw_data.py:302-353). */
int  msl_tacaw_dispersion(msl_handle* h, const void* d_src_f32, int64_t B, int64_t F, int64_t K, int64_t ld, const int64_t* idx, int64_t n,
                          float* out);
/* msl_adf: out[b] = mean_t sum_k w(k) |Psi[b,t,k]| over a (B,T,K) complex64 array (NULL: the handle's wavefunction
 *   buffer); mask = the annulus q > collection_angle*1e-3/lambda as K host bytes.
 *   Replaces the masked |.| sum and frame mean of HAADFData.calculateADF (haadf_data.py:72-94). */
int  msl_adf(msl_handle* h, const void* d_src_c64, int64_t B, int64_t T, int64_t K, int64_t ld, const uint8_t* mask, double* out);

/* ---- STEM detectors: per-image detector signals, so that a scan can stream over probe batches ----
 * msl_set_detectors: n (1..16) detectors over the handle's stored pixels (the k-window / bins, K = wx*wy of the stored spectrum):
 *   member_K = K host uint16, bit d set <=> pixel k lies in detector d (bits >= n are ignored); signal_n = n MSL_DET_* values;
 *   kx_wx / ky_wy = the stored k axes (wx and wy floats, WFData.kxs / kys).  Uploaded once; MSL_ERR_INVALID for n outside [1, 16]
 *   or an unknown signal.
 * msl_detect: out[(b*count + j)*n + d] = sum_k w_d(k) f_d(Psi[b, t0+j, k]) over a (B,T,K) complex64 array with row pitch ld,
 *   f_d = |Psi|^2, |Psi| (the convention of HAADFData.calculateADF, haadf_data.py:50, 63), kx(k)|Psi|^2 or ky(k)|Psi|^2 with
 *   kx(k) = kx_wx[k / wy], ky(k) = ky_wy[k % wy].  d_src == NULL: the handle's wavefunction buffer (T = n_frames, K = stored pixels,
 *   ld = msl_result_pitch); B <= 0 there means n_probes, a smaller B leaves the last probes out (a padded probe batch).  out is HOST
 *   memory, B*count*n float64.  One launch over every row and detector plus one float64 finishing launch; fp32 partials over at most
 *   1024 pixels, float64 from there on, no atomics (bitwise reproducible).
 *   Replaces, per probe batch, the masked sums of HAADFData.calculateADF (haadf_data.py:44-94) without the (P,T,nx,ny) array. */
#define MSL_DET_INTENSITY 0
#define MSL_DET_AMPLITUDE 1
#define MSL_DET_COM_X 2
#define MSL_DET_COM_Y 3
int  msl_set_detectors(msl_handle* h, int32_t n, const uint16_t* member_K, const int32_t* signal_n, const float* kx_wx, const float* ky_wy);
int  msl_detect(msl_handle* h, const void* d_src_c64, int64_t B, int64_t T, int64_t K, int64_t ld, int32_t t0, int32_t count, double* out);

/* ---- polar detector: every exit spectrum summed into radial rings x azimuthal sectors, per probe batch ----
 * A bin map gives every stored pixel (K = wx*wy of the stored spectrum) a bin id below n_bins, or MSL_POLAR_NONE for a pixel in no bin;
 * the caller forms it (pyslice_amd/polar_data.py: polar_bins, bin = ring * sectors + sector).  Any annular, segmented or DPC detector
 * is then a sum of bins chosen after the run, where msl_detect needs its at most 16 regions before it.
 * msl_polar_layout: host only, no handle and no device.  Stable counting sort of the K pixels by bin: order_K (room for K entries) lists
 *   the pixel indices of bin 0 ascending, then bin 1, ...; pixels with MSL_POLAR_NONE are left out.  seg_n1 has n_bins + 1 entries:
 *   seg[b] .. seg[b+1] is the slice of order for bin b, seg[n_bins] the number of pixels in any bin.  MSL_ERR_INVALID for a null argument,
 *   K < 0, n_bins outside [1, MSL_POLAR_MAX_BINS] or a bin id >= n_bins other than MSL_POLAR_NONE.
 * msl_set_polar: bin_K = K host uint16 over the handle's stored pixels; runs the layout and uploads order and seg (4 * K + 8 * (n_bins + 1)
 *   bytes on the device).  Same errors; a failed call leaves no map set.
 * msl_polar_detect: out[(b*count + j)*n_bins + i] = sum over the pixels k of bin i of |Psi[b, t0+j, k]|^2 over a (B,T,K) complex64 array with
 *   row pitch ld.  Source arguments as msl_detect: d_src == NULL is the handle's wavefunction buffer (T = n_frames, K = stored pixels,
 *   ld = msl_result_pitch; B <= 0 means n_probes, a smaller B leaves the padded probes out).  out is HOST memory, B*count*n_bins float64;
 *   the device stages it in 8 * B*count*n_bins bytes of scratch.  MSL_ERR_STATE before msl_set_polar; MSL_ERR_INVALID when K is not the K
 *   of the map, ld < K, count < 1 or [t0, t0+count) leaves [0, T).  One launch, a bin-sorted gather: one wave per bin and block of rows,
 *   fp32 |Psi|^2 added in float64 in the order of the layout, a fixed xor tree over the wave; the pad pixels [K, ld) are never read; an
 *   empty bin gives exactly 0; no atomics (bitwise reproducible).
 *   Not in the reference, which holds every frame: there the same numbers are masked sums of |wavefunction_data|^2. */
#define MSL_POLAR_NONE 0xFFFF
#define MSL_POLAR_MAX_BINS 4096
int  msl_polar_layout(const uint16_t* bin_K, int64_t K, int32_t n_bins, uint32_t* order_K, int64_t* seg_n1);
int  msl_set_polar(msl_handle* h, int32_t n_bins, const uint16_t* bin_K);
int  msl_polar_detect(msl_handle* h, const void* d_src_c64, int64_t B, int64_t T, int64_t K, int64_t ld, int32_t t0, int32_t count, double* out);

/* ---- spectrum detectors: energy-resolved detector signals of a TACAW intensity, per probe batch ----
 * msl_spectrum_detect: out[(b*count + j)*n + d] = sum_k w_d(k) I[b, f0+j, k] over a (B,F,K) float32 intensity with row pitch ld (0: K),
 *   w_d the memberships of the n detectors of the last msl_set_detectors: every detector in ONE pass over the intensity, where
 *   msl_tacaw_spectrum takes one pass and one host round trip per mask.  d_src == NULL: the handle's intensity buffer as left by
 *   msl_tacaw / msl_tacaw_layer / a finished stream (F its frequency count, K = stored pixels, ld its own pitch); B <= 0 there means
 *   n_probes, a smaller B leaves the last probes out (a padded probe batch).  out is HOST memory, B*count*n float64.
 *   MSL_ERR_STATE without detectors, or with d_src == NULL and no intensity.  MSL_ERR_INVALID when a detector's signal is not
 *   MSL_DET_INTENSITY (an amplitude or centre-of-mass weight of a TACAW intensity is not defined here), when K is not the K of the
 *   detector set-up, ld < K, count < 1 or [f0, f0+count) leaves [0, F).  One launch over every row and detector plus the float64
 *   finishing launch of msl_detect; 16-byte loads when ld % 4 == 0 and the base is 16-byte aligned (else 8 or 4 bytes), the pad
 *   pixels [K, ld) are never read; fp32 partials over at most 1024 pixels (non-negative addends), float64 from there on, no atomics
 *   (bitwise reproducible).
 *   Replaces, per probe batch, the loop of TACAWData.spectrum_image (tacaw_data.py:145-179) over a (P,F,nx,ny) array. */
int  msl_spectrum_detect(msl_handle* h, const void* d_src_f32, int64_t B, int64_t F, int64_t K, int64_t ld, int32_t f0, int32_t count, double* out);

/* ---- diffraction patterns: frame-summed |Psi|^2 on a pixelated detector (CBED / 4D-STEM), per probe batch ----
 * msl_diffract: out[(b*mx + ix)*my + iy] = sum_{j<count} sum_{a<bx} sum_{c<by} |Psi[b, t0+j, (ix*bx+a)*wy + iy*by+c]|^2 over a (B,T,K = wx*wy)
 *   complex64 array with row pitch ld, mx = wx/bx, my = wy/by: the SUM over the count frame slots (the caller divides for the
 *   frozen-phonon mean) of the intensity in every bx x by detector pixel.  Source arguments as msl_detect: d_src == NULL is the handle's
 *   wavefunction buffer (T = n_frames, K = stored pixels, ld = msl_result_pitch, wx x wy must be the stored window, B <= 0 means
 *   n_probes, a smaller B leaves the padded probes out).  out is HOST memory, B*mx*my float64.  MSL_ERR_INVALID when bx does not
 *   divide wx or by not wy, wx*wy != K, ld < K, or [t0, t0+count) leaves [0, T).  Needs no set-up and keeps no state.
 *   One launch, every complex value read once; fp32 |Psi|^2 and fp32 partial sums of at most 8 addends, float64 from there on, no
 *   atomics (bitwise reproducible).  Unlike bin_nx / bin_ny of the configuration, which add complex pixels, these bins add intensities. */
int  msl_diffract(msl_handle* h, const void* d_src_c64, int64_t B, int64_t T, int64_t K, int64_t ld, int32_t t0, int32_t count, int32_t wx, int32_t wy,
                  int32_t bx, int32_t by, double* out);

/* ---- coherent frame sums: the elastic part |<Psi>|^2 of a frozen-phonon run, per probe batch ----
 * The handle owns one accumulator, (B, pitch) float64 complex with pitch = msl_result_pitch's value (stored pixels rounded up to 32), 16 * pitch
 * bytes per probe, freed with the handle.
 * msl_coherent_reset: sizes the accumulator for B probes (B <= 0: n_probes; it only grows) and zeroes it on the handle's stream.
 * msl_coherent_add: acc[b, k] += sum_{j<count} Psi[b, t0+j, k] for k < K, over a (B,T,K) complex64 array with row pitch ld.  Source
 *   arguments as msl_detect: d_src == NULL is the handle's wavefunction buffer (B <= 0 means n_probes, a smaller B leaves the padded
 *   probes out).  MSL_ERR_INVALID when ld < K, when [t0, t0+count) leaves [0, T), when B or K exceeds what the last reset sized (K > pitch)
 *   or when K differs from the K of an earlier add since the reset.  One launch, queued on the stream (no wait); every complex value
 *   read once and widened to float64 BEFORE it is added, the frames in order, no atomics: the sum does not depend on how the frames are
 *   split over calls, and repeated sequences are bitwise equal.
 * msl_coherent_finish: out[(b*mx + ix)*my + iy] = sum_{a<bx} sum_{c<by} |acc[b, (ix*bx+a)*wy + iy*by+c]|^2 / n^2, mx = wx/bx, my = wy/by:
 *   with n = the number of frames added (n >= 1), |mean over the frames of Psi|^2 summed over every bx x by detector pixel -- the
 *   coherent mean first, the bin adds intensities as msl_diffract's.  out is HOST memory, B*mx*my float64 (B <= 0: the B of the last
 *   reset).  MSL_ERR_INVALID when bx does not divide wx or by not wy, when wx*wy is not the K of the adds, for n < 1 or B beyond the
 *   last reset.  The accumulator is left as it is.
 *   Not in the reference, which holds every frame: there the same numbers are |wavefunction_data.mean(frame axis)|^2. */
int  msl_coherent_reset(msl_handle* h, int64_t B);
int  msl_coherent_add(msl_handle* h, const void* d_src_c64, int64_t B, int64_t T, int64_t K, int64_t ld, int32_t t0, int32_t count);
int  msl_coherent_finish(msl_handle* h, int64_t B, int32_t n, int32_t wx, int32_t wy, int32_t bx, int32_t by, double* out);

/* ---- finite dose: Poisson counts of the frame-summed patterns of a probe batch, drawn on the device ----
 * The handle owns one accumulator, (B, mx*my) float64, and a uint32 staging of the counts; both only grow and are freed with the handle.
 * msl_dose_reset: sizes the accumulator for B probes (B <= 0: n_probes) of mx x my detector pixels and zeroes it on the handle's stream.
 *   MSL_ERR_INVALID for mx < 1 or my < 1.
 * msl_dose_add: acc[b, ix*my + iy] += msl_diffract's out[(b*mx + ix)*my + iy], with msl_diffract's arguments, reads, bin modes and
 *   summation order; one launch, queued on the stream (no wait), no atomics: the calls since the reset are added in call order, and
 *   repeated sequences are bitwise equal.  MSL_ERR_STATE before a reset; MSL_ERR_INVALID for what msl_diffract refuses (a bin that does
 *   not divide the window ...), for B beyond the reset and for wx/bx x wy/by other than the reset's mx x my.
 * msl_dose_counts: counts_out[b*mx*my + i] = the Poisson draw of lam = acc[b, i] * scale (one float64 multiply) from the stream of
 *   pixel i, probe probe0 + b under the 64-bit key seed: Philox-4x32-10 with the counter (i, probe0 + b, attempt, 0), inversion below
 *   lam = 10 and Hoermann's PTRS from there on, every loop bounded -- the definition, word for word, is pyslice_amd/dose.py.  scale is
 *   the electrons per unit of the accumulator, N_e / I_incident for the accumulator's frame SUM over n frames divided by n:
 *   N_e / (n * I_incident).  One launch, one thread per pixel; the counts go to the device staging and from there to counts_out, HOST
 *   memory of B*mx*my uint32 (B <= 0: the B of the reset); with intensity_out != NULL the accumulator itself is copied there, HOST
 *   memory of B*mx*my float64.  Counts saturate at 2^32 - 1.  MSL_ERR_STATE before a reset; MSL_ERR_INVALID for B beyond the reset, a
 *   negative or non-finite scale, probes outside [0, 2^32) and for a lam that is negative or not finite (found by the kernel; the
 *   outputs are then not to be used).  The accumulator is left as it is.
 *   Not in the reference, which returns noise-free intensities. */
int  msl_dose_reset(msl_handle* h, int64_t B, int32_t mx, int32_t my);
int  msl_dose_add(msl_handle* h, const void* d_src_c64, int64_t B, int64_t T, int64_t K, int64_t ld, int32_t t0, int32_t count, int32_t wx, int32_t wy,
                  int32_t bx, int32_t by);
int  msl_dose_counts(msl_handle* h, int64_t B, double scale, uint64_t seed, int64_t probe0, uint32_t* counts_out, double* intensity_out);

/* ---- member ensembles: the patterns of the G member probes of every scan position folded on the device (partial coherence) ----
 * The B waves of the source are Q = B / G positions of G members each, wave b = q*G + g; weights = G doubles on the HOST, each finite
 * and >= 0 (the caller normalises them); they travel with the launch as kernel arguments and are not read after the call returns.
 * msl_diffract_members: out[(q*mx + ix)*my + iy] = sum_{g<G} weights[g] * D[q*G + g, ix, iy], D being msl_diffract's result for that
 *   wave with the same arguments: its loads, its fp32 partial sums of at most 8 addends, its bin modes and owner lanes; the product
 *   and the sum over g are float64, each rounded on its own, in member order -- bit for bit the host's fold of msl_diffract's output,
 *   and with G = 1, weights = {1} msl_diffract itself.  One launch, every complex value read once, no atomics.  out is HOST memory,
 *   Q*mx*my float64.  MSL_ERR_INVALID for G outside [1, MSL_MEMBERS_MAX], B not a multiple of G, a negative or non-finite weight and
 *   everything msl_diffract refuses.
 * msl_dose_add_members: the same totals ADDED to the accumulator of msl_dose_reset, which was sized for (at least) Q positions, as
 *   msl_dose_add adds msl_diffract's; msl_dose_counts / msl_dose_frames then run as they are, with B = Q and probe0 the index of the
 *   first position in the scan: the draw is made from the averaged pattern.  Queued on the stream like msl_dose_add (no wait).
 *   MSL_ERR_STATE before a reset; MSL_ERR_INVALID as above
 *   and for what msl_dose_add refuses. */
#define MSL_MEMBERS_MAX 128
int  msl_diffract_members(msl_handle* h, const void* d_src_c64, int64_t B, int64_t T, int64_t K, int64_t ld, int32_t t0, int32_t count, int32_t wx,
                          int32_t wy, int32_t bx, int32_t by, int32_t G, const double* weights, double* out);
int  msl_dose_add_members(msl_handle* h, const void* d_src_c64, int64_t B, int64_t T, int64_t K, int64_t ld, int32_t t0, int32_t count, int32_t wx,
                          int32_t wy, int32_t bx, int32_t by, int32_t G, const double* weights);

/* ---- images through an objective lens (HRTEM, focal series): frame-accumulated |psi|^2 in the image plane, per probe batch ----
 * For probe b and the frames j of a call
 *     I[first + b*stride](r) += weight * sum_{j<count} | ifft2( ifftshift(Psi[b, t0+j]) * H )(r) |^2,
 *     H(k) = A(k) exp(-i chi(k)),   A(k) = 1 for |k| < aperture_k (strict, the rule of msl_set_probes) or without an aperture, else 0,
 * with Psi the stored exit spectrum fftshift(fft2(exit)), unnormalised, ifft2 NumPy's (1/(nx*ny)), and chi the aberration function of
 * msl_set_aberrations: the same fourteen terms, order and sign, evaluated in float64 on the device.  Sign of defocus: C10 = +dz gives
 * H = exp(-i pi lambda dz k^2), the Fresnel factor of the slice loop (multislice.py:262-275), so the image at C10 = +dz is the intensity
 * a distance dz DOWNSTREAM of the exit surface -- the opposite of abTEM's defocus = -C10, as for the probe.  A focal series is one call
 * per defocus, a focal spread one call per quadrature node with its weight; the caller divides by the number of frames.
 * The handle owns one accumulator, (n_images, nx*ny) float64, dense, freed with the handle.
 * msl_image_reset: sizes the accumulator for n_images images (it only grows) and zeroes it on the handle's stream.
 * msl_image_add: source arguments as msl_detect over a (B,T,K = nx*ny) complex64 array with row pitch ld (0: K): d_src == NULL is the
 *   handle's wavefunction buffer (B <= 0 means n_probes, a smaller B leaves the padded probes out).  polar14x2 has the layout of
 *   msl_set_aberrations (NULL: chi = 0); aperture_k in 1/Angstrom (<= 0: no aperture).  Probe b goes to accumulator image first + b*stride.
 *   Three launches per chunk of frames, queued on the stream (no wait): the lens into the work buffer of the slice loop, the inverse
 *   transform in place, the accumulation -- fp32 |psi|^2 widened to float64, times weight, added in frame order, no atomics: without
 *   a focal spread the sum does not depend on how the frames are split over calls, and repeated sequences are bitwise equal.  The work
 *   buffer holds n_probes x frame_batch images: when B*count exceeds that, the call walks the frames in chunks that fit.  MSL_BUF_EXIT
 *   is consumed (msl_download of it is MSL_ERR_STATE until the next msl_propagate).
 *   MSL_ERR_INVALID for a handle with a k-window or bins, ld < nx*ny, [t0, t0+count) outside [0, T), count < 1, non-finite polar, weight or
 *   aperture_k, stride < 0 (or 0 with B > 1), first + (B-1)*stride beyond the last reset, B above the images of the work buffer;
 *   MSL_ERR_STATE with d_src == NULL and no result ring.
 * msl_image_download: images [first, first+n) to HOST memory, n*nx*ny float64, dense; waits for the stream.
 *   Not in the reference, which has no imaging mode. */
int  msl_image_reset(msl_handle* h, int64_t n_images);
int  msl_image_add(msl_handle* h, const void* d_src_c64, int64_t B, int64_t T, int64_t ld, int32_t t0, int32_t count,
                   const double* polar14x2, double aperture_k, double weight, int64_t first, int64_t stride);
int  msl_image_download(msl_handle* h, int64_t first, int64_t n, double* out);

/* ---- PRISM (Ophus 2017): plane-wave S-matrix and probe synthesis, for scans of many probe positions ----
 * The slice loop is linear in the incident wave and applies no band limit, so a probe is a sum of plane waves, one per reciprocal-lattice
 * point inside its aperture.  With the unshifted pixel (mx, my), h = its signed index (fftfreq order) and k = h / (n d):
 *   beams:  the pixels with hx % fx == 0, hy % fy == 0 and sqrt(kx^2 + ky^2) < mrad * 1e-3 / lambda (strict, float64: the rule of
 *           msl_set_probes), in row-major order of (mx, my); Bm of them.
 *   S_b  =  Propagate(pw_b) through the current transmission stack, pw_b[i, j] = exp(2 pi i (hx i / nx + hy j / ny)).
 *   c[p,b] = (fx fy / (nx ny)) exp(2 pi i [hx (floor(nx/2)/nx + px/Lx) + hy (floor(ny/2)/ny + py/Ly)]) exp(-i chi(k_b)),
 *           chi the aberration function of msl_set_aberrations (zero when cleared).
 *   psi_p(r) = W_p(r) sum_b c[p,b] S_b(r),  W_p = 1 on the (nx/fx) x (ny/fy) periodic window centred on pixel
 *           ((-floor(nx/2) - rint(px/dx)) mod nx, likewise y) -- where the probe of msl_set_probes peaks -- and 0 elsewhere:
 *           pixel i is inside when ((i - cx + floor(wx/2)) mod nx) < wx, wx = nx/fx.
 * At f = (1, 1) psi_p is the exit wave msl_set_probes + msl_propagate give (to fp32 rounding); at f > 1 it is PRISM's approximation.
 * msl_smatrix_begin:  enumerates the beams and allocates S, (Bm, nx, ny) c64, and c.  MSL_ERR_INVALID for mrad <= 0, f < 1 or f not
 *   dividing its axis; MSL_ERR_NOMEM when S does not fit.  A second begin replaces the first.
 * msl_smatrix_beams:  returns Bm (MSL_ERR_STATE before begin) and, when hxhy is not NULL, fills Bm x 2 signed indices (hx, hy).
 * msl_smatrix_build:  propagates the beams, in chunks of n_probes, through the current potential into S (one unfused slice loop per
 *   chunk, counted in the counters).  MSL_ERR_STATE without a potential or before begin.  Overwrites the probe buffer (probes must be
 *   set again before msl_propagate) and MSL_BUF_EXIT.  Call it again after every new potential.
 * msl_smatrix_probes: c, psi_p and fftshift(fft2(psi_p)) -- on the full grid, zeros outside the window -- into frame slot `slot` of the
 *   result, k-window and binning as for msl_propagate_frame: every consumer of the result (msl_detect, msl_diffract, msl_tacaw, the
 *   downloads) works on it with the normalisation of a multislice run.  The pixels at multiples of (fx, fy) are native PRISM's pattern,
 *   the others its sinc interpolation.  xy = n_probes x 2 doubles; n_probes must be the handle's.  MSL_ERR_STATE without a built
 *   S-matrix or with n_frames == 0.  MSL_BUF_EXIT then holds psi_p; the probe buffer is overwritten and marked unset.  Four launches,
 *   queued on the stream; no atomics: repeated calls are bitwise equal.
 * msl_smatrix_probes_cropped: the same probes on PRISM's own (nx/fx) x (ny/fy) grid.  The window of probe p along x is wx = nx/fx
 *   consecutive pixels modulo nx and wx divides nx, so i -> i mod wx maps it one-to-one onto [0, wx) (likewise y).  The folded wave
 *   psi_c[i mod wx, j mod wy] = psi_p[i, j], (i, j) inside W_p, satisfies  fft2(psi_c)[m, n] = fft2(psi_p)[fx m, fy n]  exactly, with no
 *   phase ramp, because exp(-2 pi i m (i mod wx) / wx) = exp(-2 pi i (fx m) i / nx).  In stored (fftshifted) order the cropped pixel
 *   (a, b) is the full-grid pixel (floor(nx/2) + fx (a - floor(wx/2)), floor(ny/2) + fy (b - floor(wy/2))), which exists for odd and
 *   even lengths alike: the cropped spectrum is msl_smatrix_probes's taken at every (fx, fy)-th pixel, value for value, not rescaled
 *   (a sum over a region is about 1/(fx fy) of the full-grid sum: each cropped pixel stands for fx fy full ones).
 *   `src` holds the built S-matrix (its n_probes only sets the chunk of msl_smatrix_build; it may have n_frames == 0; its aberrations
 *   are the ones applied).  `dst` is an ordinary handle on the same device with nx = src.nx / fx, ny = src.ny / fy, the same dx, dy
 *   and wavelength, created without any potential (nz = 1 will do); its k-grid h / (n d) is the cropped pattern's own, so its k-window,
 *   bins, detectors and polar map apply unchanged.  n_probes must be dst's.  The coefficients run on src; the cropped synthesis writes
 *   psi_c into dst's MSL_BUF_EXIT and probe buffer (every pixel exactly once, no zero fill); dst's row transform and exit epilogue
 *   write frame slot `slot` of dst's result.  The two streams are ordered by events, both ways: dst's earlier work completes before
 *   its buffers are overwritten, the synthesis before dst's transform; no device-wide wait.  MSL_ERR_INVALID for a null argument,
 *   different devices, a dst grid that is not src's divided by its interpolation, different pixel sizes or wavelength, a probe-count
 *   mismatch, a slot out of range or a non-finite position; MSL_ERR_STATE without a built S-matrix or with dst.n_frames == 0 (errors
 *   are reported on src).  No atomics: repeated calls are bitwise equal.
 * msl_smatrix_end:    frees S, c and the beams; msl_destroy and msl_set_beam (the wavelength changes the beam set) do the same,
 *   msl_resize_probes keeps S.
 *   Not in the reference, which propagates every probe position through every slice. */
int  msl_smatrix_begin(msl_handle* h, int32_t fx, int32_t fy, double mrad);
int  msl_smatrix_beams(const msl_handle* h, int32_t* hxhy_or_null);
int  msl_smatrix_build(msl_handle* h);
int  msl_smatrix_probes(msl_handle* h, const double* xy, int32_t n_probes, int32_t slot);
int  msl_smatrix_probes_cropped(msl_handle* src, msl_handle* dst, const double* xy, int32_t n_probes, int32_t slot);
int  msl_smatrix_end(msl_handle* h);

/* ---- thickness series: spectra of intermediate layers of the stack ----
 * msl_set_layers: `n` strictly increasing slice indices k in [0, nz-1).  Layer k is the wave after the transmission of slice k and
 * before the propagation that follows it -- the exit wave of the stack cut after slice k.  Every fused slice loop then also writes
 * fftshift(fft2(layer k)) (k-window, binning and frame batching as the exit) into block l of ONE (n+1, P, T_local, pitch) c64
 * result; MSL_BUF_WAVEFUNCTION is its last block (the exit), so every call that reads the wavefunction buffer keeps working on the
 * exit wave.  The result buffer is replaced (zeros).  n = 0 restores the single-layer buffer.  MSL_ERR_INVALID for bad indices,
 * MSL_ERR_STATE with n_frames == 0 or while a stream is open, MSL_ERR_NOMEM when the device cannot hold the result.
 * The reference writes a single layer (calculators.py:221) into WFData's layer axis (wf_data.py:12-27). */
int  msl_set_layers(msl_handle* h, const int32_t* slices, int32_t n);
/* The layered result as the reference's host array (P, n_frames_used, wx, wy, L) complex128: layers interleaved and widened on
 * the device chunk by chunk, then linear copies.  dst: P * n_frames_used * wx * wy * L complex128. */
int  msl_download_layers_c128(msl_handle* h, int32_t n_frames_used, void* dst_c128, size_t bytes);
/* msl_tacaw with d_src == NULL on block `layer` of the layered result (TACAWData(wf, layer_index=layer), tacaw_data.py:61-89):
 * the intensity goes to the handle's own buffer, for the reductions with d_src == NULL. */
int  msl_tacaw_layer(msl_handle* h, int32_t layer);
/* msl_tacaw_welch with d_src == NULL on block `layer` of the layered result. */
int  msl_tacaw_welch_layer(msl_handle* h, int32_t layer, int32_t L, int32_t hop, const double* window_L);

/* ---- thickness series of the probe-batch modes: detector, polar and pattern signals of every tapped layer ----
 * msl_set_layers keeps one full block of spectra per layer; a scan that streams probe batches wants the REDUCED signals of every
 * thickness and no spectra.  Here every tap goes to ONE reused block, which is reduced at once, inside the launch sequence of the
 * slice loop, into a float64 staging area, so that device memory does not grow with the number of thicknesses.
 * msl_set_layer_reduce: `n` strictly increasing slice indices k in [0, nz-1), layer k as for msl_set_layers; the exit wave is
 *   layer n, L = n + 1.  what = MSL_LR_* bits: DETECT (the detectors of msl_set_detectors), POLAR (the bin map of msl_set_polar),
 *   DIFFRACT (patterns of bx x by stored pixels, as msl_diffract), PACBED (the same patterns summed over the probes on the device);
 *   bx, by are read with DIFFRACT or PACBED only.  Allocates the tap buffer, one block of the size of MSL_BUF_WAVEFUNCTION, the
 *   partial slab of the detector tiles, and 8 * [L * P * T * D (DETECT) + L * P * T * n_bins (POLAR) + L * P * mx * my (DIFFRACT or
 *   PACBED) + L * mx * my (PACBED)] bytes of staging, P = n_probes, T = n_frames, mx x my = the binned stored window.
 *   MSL_ERR_STATE for DETECT without detectors or POLAR without a bin map, with n_frames == 0, while a stream is open, or while
 *   msl_set_layers holds layers (and msl_set_layers is MSL_ERR_STATE while this mode is on); MSL_ERR_INVALID for bad slices, bits or
 *   bins; MSL_ERR_NOMEM with the old state intact.  n = 0 or what = 0 turns the mode off and frees the buffers.
 *   The staging has rows of the detector and bin counts of this call: while the mode is on, msl_set_detectors with another n (DETECT)
 *   and msl_set_polar with another n_bins (POLAR) are MSL_ERR_STATE; other memberships or another bin map of the same count are fine.
 *   Should a failed one of those calls leave no detectors or no map, the next slice loop is MSL_ERR_STATE and queues nothing.
 *   While the mode is on, msl_propagate_frame / msl_propagate_frames queue, behind the tap of every listed slice and behind the exit
 *   epilogue, the reductions of that layer over the frame slots of the call, for all n_probes rows (a padded probe is reduced too),
 *   with the launches of msl_detect, msl_polar_detect and msl_diffract (the frame sum covers the frames of the call) and no host
 *   synchronisation: the numbers are bit for bit those calls' on the same spectra.  MSL_BUF_LAYERS stays the single exit block.
 * msl_layer_fetch: after one stream synchronisation, the results of the last sequence for the first B probes (B <= 0: n_probes):
 *   det_out (L, B, count, D), polar_out (L, B, count, n_bins), pattern_out (L, B, mx, my) float64 HOST memory, each NULL when not
 *   wanted; count must be the frame count of that sequence.  MSL_ERR_INVALID for an output whose reduction is not on (patterns are
 *   fetched with DIFFRACT only); MSL_ERR_STATE before the first sequence.
 * msl_layer_pacbed_reset / _add / _download (PACBED): the accumulator (L, mx, my) float64 is zeroed; receives, per layer, the sum
 *   over the first B probes of the patterns of the last sequence -- one launch, float64, in probe order, no atomics: repeated runs are
 *   bitwise equal; is copied to HOST memory (waits for the stream).  reset and add are queued.
 * msl_layer_reduce_bytes: bytes of the block, the tap buffer or the staging area (MSL_LR_BYTES_*), 0 while the mode is off.
 *   Not in the reference, which holds every frame of a single layer. */
#define MSL_LR_DETECT 1u
#define MSL_LR_POLAR 2u
#define MSL_LR_DIFFRACT 4u
#define MSL_LR_PACBED 8u
#define MSL_LR_BYTES_BLOCK 0
#define MSL_LR_BYTES_TAP 1
#define MSL_LR_BYTES_STAGING 2
int  msl_set_layer_reduce(msl_handle* h, const int32_t* slices, int32_t n, uint32_t what, int32_t bx, int32_t by);
int  msl_layer_fetch(msl_handle* h, int64_t B, int32_t count, double* det_out, double* polar_out, double* pattern_out);
int  msl_layer_pacbed_reset(msl_handle* h);
int  msl_layer_pacbed_add(msl_handle* h, int64_t B);
int  msl_layer_pacbed_download(msl_handle* h, double* out);
size_t msl_layer_reduce_bytes(const msl_handle* h, int32_t which);

/* Copy a device buffer to the host (dst must hold `bytes` = full buffer size, see msl_buffer_bytes).
 * For MSL_BUF_WAVEFUNCTION / MSL_BUF_INTENSITY the host copy is dense -- (P,T,wx,wy), bytes = P*T*wx*wy*8 or *4, the pixel
 * pitch of the device buffer (msl_result_pitch) is dropped on the way -- and `first`/`count` select a probe range (count==0: all).
 * MSL_BUF_LAYERS: dense (L,P,T,wx,wy), no range. */
int  msl_download(msl_handle* h, msl_buffer what, void* dst, size_t bytes, int64_t first, int64_t count);
/* The (P, T_local, nx, ny) result as complex128 -- the dtype the reference returns (calculators.py:161, 284-290: its arrays are
 * torch.complex128) -- for the frames [0, n_frames_used) of every probe: widened on the device chunk by chunk and copied out as
 * 16 B per element, instead of a complex64 download followed by a single-threaded astype on the host.
 * dst_c128: host, n_probes * n_frames_used * wx * wy complex128. */
int  msl_download_wavefunction_c128(msl_handle* h, int32_t n_frames_used, void* dst_c128, size_t bytes);
size_t msl_buffer_bytes(const msl_handle* h, msl_buffer what);
/* Pixel pitch of the images of MSL_BUF_WAVEFUNCTION / MSL_BUF_INTENSITY: wx*wy rounded up to a multiple of 32 pixels, so that
 * every (probe, frame) image starts on a 256-byte (c64) / 128-byte (f32) boundary and the time kernels of msl_tacaw read and
 * write whole lines on grids with odd pixel counts too (the reference's own test grid is 501 x 491, 00_probe.py:7-8; its
 * time FFT runs over exactly such arrays, tacaw_data.py:94-96).  The pad pixels hold zeros.  msl_download*, msl_*_frame and the
 * reductions with d_src == NULL hide the pitch; a caller that takes msl_device_ptr() builds its view with it.
 * The intensity buffer written by msl_tacaw_stream_finish is dense (pitch = wx*wy).  Other buffers: 0. */
int64_t msl_result_pitch(const msl_handle* h, msl_buffer what);
/* Raw device pointer of a library buffer, for zero-copy use by the caller's collective (RCCL). */
void* msl_device_ptr(msl_handle* h, msl_buffer what);

/* One frame slot of the (P,T_local,nx,ny) result, host (P,nx,ny) c64 <-> device.  Used by the opt-in frame cache
 * (reference: psi_data/torch_<key>/frame_<i>.npy written and re-read per frame, calculators.py:173, 259-260, 311). */
int  msl_download_frame(msl_handle* h, int32_t slot, void* dst_c64, size_t bytes);
int  msl_upload_frame(msl_handle* h, int32_t slot, const void* src_c64, size_t bytes);

/* Wait for everything queued on the handle's stream. */
int  msl_synchronize(msl_handle* h);
int  msl_get_counters(const msl_handle* h, msl_counters* out);
int  msl_reset_counters(msl_handle* h);

/* Batched 2-D FFT self-test entry (parity tests of the FFT kernels alone): in/out host (B,nx,ny) c64,
 * dir=+1 forward / -1 inverse (1/(nx*ny) normalised), path as msl_config.fft_path. */
int  msl_fft2_host(msl_handle* h, const float* in_c64, float* out_c64, int32_t batch, int32_t dir);

/* ---- finite projection: atomic potentials spread over neighbouring slices ----
 * Without it every build is an infinite projection: the whole projected form factor f_Z(k^2) of an atom goes to the one slice whose
 * [lo, hi) holds its z.  With reach_slices = R > 0 and nodes = J every later msl_build_potential / msl_build_potentials /
 * msl_build_thermal / msl_build_modes deposits in slice s the part of the atom's 3D Kirkland potential that lies in that slice
 * (pyslice_amd/projection.py is the definition):
 *   - slabs are uniform, slab s = [e0 + s dz, e0 + (s+1) dz) with dz the handle's dz and e0 = c_0 - dz/2 the lower edge the reference's
 *     slice rule gives the interior slices (taken from the edges of msl_set_slices: lo[1] - dz; with one slice hi[0] - 3 dz / 2);
 *   - each slab holds J node planes at spacing h = dz / J; an atom at z becomes two partial atoms on the nodes n0 = floor((z - e0) / h)
 *     and n0 + 1 with the weights 1 - w and w, w = (z - e0) / h - n0 (total and z-centroid kept; w = 0: one atom);
 *   - node n gives slab s, m = n - s J in [-R J, (R+1) J), the in-plane transform of the slab zeta in [-m h, -m h + dz) of the atom,
 *         F_Z(k; a, b) = sum_j a_j / (2 kappa_j^2) [S(b, kappa_j) - S(a, kappa_j)] + c_j exp(-d_j k^2) 1/2 [erf(pi b / sqrt d_j) - erf(pi a / sqrt d_j)],
 *         kappa_j = sqrt(k^2 + b_j),  S(zeta, kappa) = sgn(zeta) (1 - exp(-2 pi kappa |zeta|)),
 *     with a = -infinity in the lowest slab reached and b = +infinity in the highest: the 2 R + 1 tables of a node sum to f_Z(k^2);
 *   - an atom counts iff it counts without the option (lo[0] <= z < hi[nz-1], known species); what it would give to slabs below 0 or
 *     above nz - 1 is dropped (as an atom that leaves the stack is dropped).
 * The build makes n_species (2 R + 1) J channel tables (MSL_BUF_FORMFACTOR_FINITE) once per species list, and 2 (2 R + 1) weighted
 * rows per atom through the sort, the phase tables and the structure factor of the ordinary build; the inverse transform and the
 * slice loop are unchanged.  reach_slices = 0 (the default; nodes is then only stored) turns it off: the builds of a handle the call
 * was never made on, bit for bit.  Every change of (R, J) makes the next build compute its tables again.
 * MSL_ERR_INVALID: nodes outside [1, 16], reach_slices outside [0, 32].  MSL_ERR_UNSUPPORTED: while msl_set_absorption, msl_set_tds
 * or msl_set_ionization is set (and msl_set_absorption is MSL_ERR_UNSUPPORTED while this is on); at build time, when an interior slice is not dz thick.
 * msl_get_projection: reach_nodes[0..1] = (reach_slices, nodes), (0, 1) before the first call.  Not in the reference. */
int  msl_set_projection(msl_handle* h, int32_t reach_slices, int32_t nodes);
int  msl_get_projection(const msl_handle* h, int32_t* reach_nodes);

/* ---- detector response: point spread, gain, dark offset, readout noise, uint16 frames ----
 * What a camera writes for the electron counts of a probe batch; the definition, word for word, is pyslice_amd/camera.py.  For pixel
 * (ix, iy) of the mx x my pattern of probe p, with c the counts as float64 and zero outside the pattern:
 *     s = 0;  for a = -r .. r:  for b = -r .. r:  s = s + psf[(a+r)*(2r+1) + (b+r)] * c[ix-a, iy-b]      (a convolution, zero boundary)
 *     e = gain * s;  e = e + offset;  readout_noise > 0 only:  e = e + readout_noise * sqrt(-2 ln u) * cos(2 pi v)
 *     frame = clip(rint(e), 0, 2^bits - 1) as uint16
 * every product and sum rounded on its own in float64; (u, v) = U(x0, x1), U(x2, x3) of Philox-4x32-10 under the 64-bit key seed with
 * the counter (ix*my + iy, p, 0, 1) -- word 3 = 1, the Poisson draws of msl_dose_counts use 0 -- and the U of msl_dose_counts.
 * msl_set_camera: copies the (2 radius + 1)^2 weights (HOST memory, row-major [a+r][b+r]; NULL only with radius 0: the weight 1) to the
 *   device and stores the scalars.  radius < 0 clears the camera.  MSL_ERR_INVALID for a radius above 8, a NULL table with radius > 0, a
 *   negative or non-finite weight, a gain not finite and > 0, a negative or non-finite offset or readout_noise, bits outside 1 .. 16;
 *   the camera set before is then kept.  Touches nothing else on the handle.
 * msl_camera_frames: uploads B*mx*my counts from HOST memory into the count staging of msl_dose_counts, runs the pass for the probes
 *   probe0 .. probe0 + B - 1 (one launch) and downloads B*mx*my uint16 to frames_out, HOST memory.  MSL_ERR_STATE without a camera;
 *   MSL_ERR_INVALID for a NULL pointer, B < 1, mx < 1 or my < 1, probes outside [0, 2^32).  The accumulator of msl_dose_reset is not touched.
 * msl_dose_frames: the draw of msl_dose_counts into the staging (its arguments, checks and flag word) and the pass on the same stream,
 *   then one download of 2 bytes per pixel to frames_out; the counts (B*mx*my uint32) and the accumulator (B*mx*my float64) come back
 *   only where their pointers are not NULL.  MSL_ERR_STATE before a msl_dose_reset or without a camera.
 * Without readout noise the frames are the definition's bit for bit; with it they may differ by one unit where the device's log, sqrt
 * or cos differ from the host's in the last place and e lies that close to a half-integer.  Not in the reference. */
int  msl_set_camera(msl_handle* h, int32_t radius, const double* psf, double gain, double offset, double readout_noise, int32_t bits);
int  msl_camera_frames(msl_handle* h, const uint32_t* counts_host, int64_t B, int32_t mx, int32_t my, uint64_t seed, int64_t probe0, uint16_t* frames_out);
int  msl_dose_frames(msl_handle* h, int64_t B, double scale, uint64_t seed, int64_t probe0, uint16_t* frames_out, uint32_t* counts_out_or_null,
                     double* intensity_out_or_null);

#ifdef __cplusplus
}
#endif
#endif /* MSLICE_H */
