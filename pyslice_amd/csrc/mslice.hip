// libmslice: C-ABI HIP implementation of the multislice hot path for MI355X (gfx950).
// Entry points are declared in include/mslice.h (each cites the reference function it replaces).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/mslice.h"
#include "fft_generic.h"
#include "fft_pow2.h"
#include "pot_ifft.h"
#include "rowtm_pass.h"
#include "potential.h"
#include "absorptive.h"
#include "finite.h"
#include "tds.h"
#include "ionization.h"
#include "slice_sums.h"
#include "adjoint.h"
#include "thermal.h"
#include "phonons.h"
#include "reduce.h"
#include "stream.h"
#include "tacaw_time.h"
#include "tacaw_launch.h"
#include "tacaw_welch.h"
#include "layer_tap.h"
#include "layer_reduce.h"
#include "detect.h"
#include "polar.h"
#include "spectrum_detect.h"
#include "diffract.h"
#include "ensemble.h"
#include "coherent.h"
#include "dose.h"
#include "camera.h"
#include "image.h"
#include "smatrix.h"
#include "propagator.h"
#include "bandlimit.h"

using namespace msl;

namespace {

thread_local std::string g_create_error;

int fail(msl_handle* h, int code, const char* fmt, ...);

// Device memory of n elements of T with one owner: freed by the destructor, moved but never copied.  Reads as a T* wherever a
// pointer is wanted (arithmetic, job structs, kernel arguments).  Every device allocation of this file is a DevBuf.
template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept { std::swap(p, o.p); std::swap(n, o.n); return *this; }
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    operator T*() const { return p; }
    void release() { if (p) (void)hipFree(p); p = nullptr; n = 0; }
    // free, then allocate exactly `count` elements (0: stays empty); on failure the buffer is empty and the handle's error is set
    int alloc(msl_handle* h, size_t count) {
        release();
        if (count == 0) return MSL_OK;
        hipError_t e = hipMalloc((void**)&p, count * sizeof(T));
        if (e != hipSuccess) { p = nullptr; return fail(h, MSL_ERR_NOMEM, "hipMalloc(%zu bytes) failed: %s", count * sizeof(T), hipGetErrorString(e)); }
        n = count;
        return MSL_OK;
    }
    int reserve(msl_handle* h, size_t count) { return count <= n ? MSL_OK : alloc(h, count); }     // grow only
};

struct FftPlan {
    int M = 0;                  // length the Stockham stages run on (N, or a power of two >= 2N-1: Bluestein)
    DevBuf<float2> chirp, bfilt;
    int N = 0;
    int n_stages = 0;
    int radix[MSL_MAX_STAGES] = {0};
    DevBuf<float2> tw;          // device twiddles
    bool ok = false;
};

enum LaunchKind { K_ROW = 0, K_COL = 1, K_OTHER = 2, K_NKINDS = 3 };

// What the slice loop runs along one axis (plan_axis_kind), and the tables of msl_handle::OpDir each kind reads:
//   AX_FOURSTEP  R^2 = 256 / 1024 points, the four-step register kernel (tw4_x / tw4_y)
//   AX_TWO       2 R^2 = 512 points (tw = the R^2 table, tw2 = W_512^m, ptab = the split-order Fresnel table)
//   AX_WAVE2K    2048 points, one wave per line (tw = T[k1*64+n2], tw2 = W_64)
//   AX_MIXED     smooth length A * B or 2 A * B on rowTM_pass_kernel (mtw = its two twiddle tables)
//   AX_CONV      any length <= R^2/2: the propagation as a zero-padded cyclic convolution on the R^2 register FFTs (filter qf, cz)
//   AX_CONV2K    513..1024 points: the same on the wave-per-line 2048-point FFT (filter qf, cz)
//   AX_CONV4K    1025..2047 points: cyclic convolution of length 4096 (tw, tw2 as AX_WAVE2K, bw = W_4096^i, qf in rowTC2's split order)
//   AX_GENERIC   the generic LDS kernel with a transposing store
enum AxisKind { AX_NONE, AX_FOURSTEP, AX_TWO, AX_WAVE2K, AX_MIXED, AX_CONV, AX_CONV2K, AX_CONV4K, AX_GENERIC };

// How the potential build inverse-transforms the structure factors and applies exp(i sigma V) (plan_pot_ifft, potential_ifft):
//   PI_LINES   in place, each axis on its own: the four-step kernel where the axis has one (Ry / Rx), launch_lines otherwise
//   PI_TWO     512 x 512 (both axes AX_TWO): ifftT2_kernel
//   PI_CHIRPZ  chirp-z tables along both axes (OpDir::cz): ifftTB_two / ifftTB / ifftTB2_kernel
//   PI_WAVE2K  2048 x 2048 (both axes AX_WAVE2K): ifftTW_kernel
enum PotIfft { PI_LINES, PI_TWO, PI_CHIRPZ, PI_WAVE2K };

// Chirp-z tables of n points on a register FFT of length M: R = 16 / 32 (M = R^2, tw = make_tw4's table) or 64 (the wave-per-line
// 2048-point FFT: tw = T[k1*64+n2], tw2 = W_64), chirp bw (M/2 entries) and its filter bf (M/2 + 2), made by make_cz_tables.  The
// convolution passes of the slice loop, the potential's inverse transform (ifftTB_kernel / ifftTB2_kernel) and time_cz_kernel read them.
struct CzTables { int R = 0; DevBuf<float2> tw, tw2, bf, bw; };

struct EventSet {
    std::vector<hipEvent_t> ev;
    std::vector<int> kind;      // kind[i] = kind of the launch between ev[i] and ev[i+1]
    int used = 0;               // number of events recorded
    bool pending = false;
};

}  // namespace

struct msl_handle {
    msl_config cfg{};
    hipStream_t stream = nullptr;
    std::string err;
    // plans
    FftPlan plan_x, plan_y, plan_t;
    // four-step (register-resident) kernels: R = 32 (N=1024) or 16 (N=256); 0 = use the generic kernel
    int Rx = 0, Ry = 0;
    DevBuf<float2> tw4_x, tw4_y;
    int n_cus = 256;
    // one-pass-per-slice path (transposing passes): second work buffer in (P, ny, nx+pad) layout, transposed
    // probes and the transposed transmission slices
    int wx = 0, wy = 0, wx0 = 0, wy0 = 0;   // k-window of the stored exit-wave spectra (fftshifted coordinates)
    size_t wpix = 0;               // stored pixels per exit-wave spectrum: the (binned) k-window or the whole grid
    size_t wpitch = 0;             // pixel pitch of the images of wf / intensity: wpix rounded up to 32 pixels (pad pixels are zero: to the
                                   // time kernels they are pixels like any other), include/mslice.h: msl_result_pitch
    size_t intensity_ld = 0;       // pixel pitch of the resident intensity buffer: wpitch after msl_tacaw, wpix after a stream
    int bx = 1, by = 1;            // detector binning: stored pixel = sum of bx x by neighbouring pixels of the window
    DevBuf<float2> bin_stage;      // binning: full-resolution window of the frames of one launch sequence, (FB*P, wx, wy)
    // streaming TACAW
    DevBuf<float2> st_acc, st_tw; DevBuf<double2> st_s1; DevBuf<double> st_s2; DevBuf<int> st_bins;
    DevBuf<float2> st_ref; bool st_have_ref = false;         // reference pattern subtracted before folding (msl_tacaw_stream_set_reference)
    int st_T = 0, st_F = 0; bool st_open = false;
    int64_t intensity_F = 0;       // frequency bins of the resident intensity buffer (T after msl_tacaw, n_bins after a stream)
    DevBuf<char> scratch;          // reductions: partial sums / masks / index lists (grown on demand)
    bool onepass = false;
    // onepass_planned: what msl_create planned; onepass: the loop that runs now -- false while a tilt lies along an axis whose one-pass
    // kernel needs an even table (set_loop_mode, the only writer of onepass and pot_ifft after msl_create).  The invariant: whatever is
    // SIZED or made once (psiT, psi0T and its transposed probes, transT, the pitches, scheme_b, need_psi0T) follows onepass_planned;
    // whatever CHOOSES launches or the order of the stored slices (slice_loop, slice_is_transposed, transpose_odd_slices,
    // restore_natural_slices, plan_pot_ifft, ifft_inplace, the transmission download) follows onepass.
    bool onepass_planned = false;
    bool scheme_b = false;         // a direction of 2R^2 points: every pass transposes, first pass along y, final transpose if nz is odd
    PotIfft pot_ifft = PI_LINES;   // inverse transform of the potential build: planned at msl_create, PI_LINES while set_loop_mode has the two-pass loop on
    // one-pass kernel of one axis (AxisKind) and its tables: n = line length, R = radix of the base kind's register FFT (0: none).
    // `base` is the kind the axis has without the mixed-radix pass (== kind otherwise): a MIXED axis keeps the tables of its base
    // kind, on which the potential's inverse transform, the probes and the exit FFT still run, and the loop is one-pass iff both
    // bases are not AX_NONE.  cz: the chirp-z tables of a CONV / CONV2K base, or of an axis of 33..1024 points next to one (only the
    // potential's inverse transform uses those).  Every table is owned by the OpDir.
    struct OpDir { AxisKind kind = AX_NONE, base = AX_NONE; int n = 0; int R = 0; DevBuf<float2> mtw, tw, tw2, qf, bw, ptab;
                   CzTables cz; } opx, opy;
    CzTables opt;                  // chirp-z tables of the TACAW time axis, made for opt_T frames (time_cz_kernel)
    int opt_T = 0;
    DevBuf<float2> tsplit_tw;      // W_T^n, n < T: cross-wave butterflies of time_split_kernel, made for tsplit_T frames
    int tsplit_T = 0;
    DevBuf<float> welch_g;         // msl_tacaw_welch: the window x normalisation table of the last call (welch_g_host, what the device holds)
    std::vector<float> welch_g_host;
    DevBuf<float2> psiT, psi0T;
    bool need_psi0T = false;
    int keys_cap = 0;              // capacity of d_counts / d_start (slice x species bins)
    // pinned host staging for the per-frame inputs (species maps, Z, positions), two slots used alternately: the call
    // copies the caller's arrays here and returns; the H2D copies run on the stream (no pointer into caller memory is kept)
    struct HostStage { char* buf = nullptr; size_t bytes = 0; hipEvent_t ev = nullptr; bool used = false; } stage[2];
    unsigned stage_pos = 0;
    DevBuf<float2> transT;
    int pitchT = 0;
    int debug_flags_mask = -1;
    int row_pchunk = 0;         // 0 = auto (MSL_ROW_PCHUNK, debug)
    int pitch = 0;              // row pitch (elements) of psi0/psi; > ny de-aliases the column pass's 128-byte segments
    // frame batching (msl_config.frame_batch): FB frames share one launch of every slice-loop kernel -- image index =
    // frame * P + probe, each frame with its own transmission stack.  Work buffers hold FB * P images (the probes are
    // replicated once per frame of the batch), trans / transT hold FB stacks; cur_batch = stack the next potential goes to.
    int FB = 1, cur_batch = 0;
    // device buffers
    DevBuf<float2> psi0, psi, trans;
    DevBuf<float> V;
    DevBuf<float> intensity;
    DevBuf<float2> pxt, pyt;    // exp(-i pi lambda dz kx^2)/nx
    // the settings that, with the beam in cfg, decide the propagator tables, the loop mode and the low-pass of the stacks (DESIGN.md
    // section 4.25) -- one value: a setter copies it, changes it, refreshes, and on a refusal puts the copy back
    struct Settings {
        double tilt_tan[2] = {0.0, 0.0};   // specimen tilt (msl_set_tilt): tan(theta) along x and y
        bool tilt_set = false;             // msl_set_tilt has been called (never cleared: (0, 0) is a tilt like any other)
        int bl_cut[2] = {-1, -1};          // band limit (msl_set_bandlimit): the largest kept |frequency index| per axis
        bool bl_on = false;                // (-1 and false: none)
    } set;
    DevBuf<double2> tilt_work;     // fill_propagator_device: the float64 tables of its convolution sums
    DevBuf<float2> bl_mx, bl_my;   // while set.bl_on: the weight vectors mask / n of bandlimit_lowpass (bandlimit.h)
    // the result, (L, P, T_local, wpitch) with L = 1 + the layers of a thickness series (msl_set_layers): `layers` owns it for every
    // L, wf is a view of its last block, the exit waves.  layer_block: result block of every slice (-1: not a layer); tap: the
    // natural-order image set the layer tap transforms (FB * P images, psi's layout); tap_cx / tap_cy: the unscaled conjugate
    // propagator factors conj(Px), conj(Py) of the tap
    std::vector<int> layer_block;
    std::vector<int> layer_slices;
    DevBuf<float2> layers;
    float2* wf = nullptr;
    DevBuf<float2> tap, tap_cx, tap_cy;
    // thickness series of the probe-batch modes (msl_set_layer_reduce, layer_reduce.h): the taps of layer_slices go to the ONE
    // block lr_block, which is reduced at once into layer l's part of the float64 staging lr_stage (layout lr_lay); `layers`
    // stays the single exit block.  lr_what: MSL_LR_* bits; lr_bx, lr_by: the bin of the patterns; lr_slot / lr_count: the frame
    // slots of the last sequence, whose results the staging holds (lr_count = 0: none)
    bool lr_on = false;
    unsigned lr_what = 0;
    int lr_bx = 1, lr_by = 1, lr_slot = 0, lr_count = 0;
    LrLayout lr_lay;
    DevBuf<float2> lr_block;
    DevBuf<double> lr_stage;
    // STEM detectors (msl_set_detectors): membership bits per stored pixel, the stored k axes, the signal of every detector
    DevBuf<uint16_t> det_mask;
    DevBuf<float> det_kx, det_ky;
    int det_n = 0, det_wy = 0;
    size_t det_K = 0;
    uint32_t det_amp = 0, det_cx = 0, det_cy = 0;
    // polar detector (msl_set_polar): the pixels sorted by bin and the bins' slices of that list (polar.h); pol_bins = 0: no map
    DevBuf<uint32_t> pol_order;
    DevBuf<long long> pol_seg;
    int pol_bins = 0;
    size_t pol_K = 0;
    // diffraction patterns (msl_diffract): (B, mx, my) float64 staging, grown on demand
    DevBuf<double> diff_out;
    // coherent frame sums (msl_coherent_reset / _add / _finish): (coh_B, wpitch) float64 complex, grown on demand; coh_K = the row
    // length of the adds since the last reset (0: none yet)
    DevBuf<double2> coh_acc;
    int64_t coh_B = 0, coh_K = 0;
    // finite dose (msl_dose_reset / _add / _counts): the (dose_B, dose_K = mx * my) float64 frame sums of a probe batch and the uint32
    // staging of their counts with the flag word behind them, both grown on demand; dose_B = 0: no reset yet
    DevBuf<double> dose_acc;
    DevBuf<uint32_t> dose_cnt;
    int64_t dose_B = 0, dose_K = 0;
    int dose_mx = 0, dose_my = 0;
    // member probes (ensemble.h): the C10 coefficient of every probe of msl_set_probe_members, grown on demand
    DevBuf<double> mem_a0;
    // detector response (msl_set_camera; camera.h): the weights padded to the radius class, the scalars of the response, and the uint16
    // staging of the frames, grown on demand; cam_radius < 0: no camera
    DevBuf<double> cam_psf;
    DevBuf<uint16_t> cam_frames;
    int cam_radius = -1, cam_class = 0, cam_bits = 16;
    double cam_gain = 1.0, cam_offset = 0.0, cam_noise = 0.0;
    // image accumulator (msl_image_reset / _add / _download): (img_n, nx * ny) float64, grown on demand
    DevBuf<double> img_acc;
    int64_t img_n = 0;
    // PRISM (msl_smatrix_*): the beams (hx, hy) on the host and the device, S (sm_Bm, nx, ny) c64 dense, the coefficients c (P, sm_Bm)
    // of the last probe batch; sm_open between begin and end, sm_built once msl_smatrix_build has filled S
    std::vector<int32_t> sm_h;
    DevBuf<int2> sm_beams;
    DevBuf<float2> sm_S, sm_c;
    int sm_fx = 0, sm_fy = 0, sm_Bm = 0;
    bool sm_open = false, sm_built = false;
    hipEvent_t sm_ev[2] = {nullptr, nullptr};      // msl_smatrix_probes_cropped, on the source: orders the two handles' streams, both ways
    DevBuf<double> d_abcd, d_lo, d_hi;
    bool have_kirkland = false, have_slices = false, have_probes = false, have_potential = false, have_exit = false;
    int frames_done = 0;
    // potential scratch (grown on demand)
    size_t atom_cap = 0;
    DevBuf<double> d_pos, d_u1, d_u2;
    DevBuf<int> d_Z, d_key, d_order, d_counts, d_start, d_z2s, d_species;
    DevBuf<float2> d_ex, d_ey;
    DevBuf<float> d_ff;
    int ff_species_cap = 0;
    int n_species = 0;
    int ff_species[104] = {0};     // species list the resident form-factor table was computed for (frame-invariant: computed once per run)
    int ff_n = 0;
    // finite projection (msl_set_projection, finite.h): reach in slices (0 = off) and nodes per slice; while it is
    // on, d_ff holds the fin_nch = species x (2 R + 1) J channel tables made for the slab thickness ff_dz, every atom becomes
    // 2 (2 R + 1) weighted rows (d_wgt next to d_u1 / d_u2) and the bins are (frame, slice, channel).  h_lo / h_hi: the host's copy of
    // the slice edges (the slab lattice and the build-time check of the interior slices)
    int fin_R = 0, fin_J = 1, fin_nch = 0;
    double ff_dz = 0.0;
    DevBuf<float> d_wgt;
    std::vector<double> h_lo, h_hi;
    // absorptive potential (msl_set_absorption, absorptive.h): the rms width per atomic number on the host and the device; while
    // abs_on, d_ff holds f D and d_ffa the absorptive tables g (abs_absorb), and every build goes through the two real stacks abs_V
    // (Vbar) and abs_O (Omega), (FB, nz, nx, ny) float32, allocated by the first such build and released when absorption is cleared.
    // abs_built: the stacks hold the potential the transmission functions were made from (msl_set_beam, the downloads)
    bool abs_on = false, abs_absorb = false, abs_built = false;
    DevBuf<double> d_abs_u;
    DevBuf<float> d_ffa, abs_V, abs_O;
    // TDS detector signal (msl_set_tds, tds.h): the memberships on the fft-order grid, the tables g_det
    // (tds_n, n_species, nx, ny) next to d_ffa, the weight stack w (tds_n, nz, nx, ny) made with the interaction constant tds_sigma,
    // the per-slice sums (nz, n_probes, tds_n) of the last slice loop (tds_have) and the slab of its partials.  While tds_on the
    // handle runs slice_loop with the split row step and the reduction between its halves, on the two-pass loop (set_loop_mode)
    bool tds_on = false, tds_have = false;
    int tds_n = 0;
    double tds_sigma = 0.0;
    DevBuf<uint16_t> tds_bits;
    DevBuf<float> tds_g, tds_W;
    DevBuf<double> tds_acc, tds_part;
    // element maps (msl_set_ionization, ionization.h): the channels (atomic number, width, cross-section),
    // their tables (ion_n, n_species, nx, ny) for the species list ion_species (ion_nsp = 0: to be made), the weight stack W
    // (ion_n, nz, nx, ny) of the last build (ion_built), an image of ones for the norm of the incident waves, the per-slice sums
    // (nz, n_probes, ion_n) and the norms (n_probes) of the last slice loop (ion_have) and the slab of its float32 partials.  While
    // ion_on the handle runs slice_loop as it does while tds_on, on the two-pass loop (set_loop_mode)
    bool ion_on = false, ion_built = false, ion_have = false;
    int ion_n = 0, ion_Z[ION_MAX] = {0}, ion_species[104] = {0}, ion_nsp = 0;
    double ion_width[ION_MAX] = {0}, ion_cross[ION_MAX] = {0};
    DevBuf<float> ion_tab, ion_W, ion_ones, ion_part;
    DevBuf<double> ion_acc, ion_norm;
    // gradients (msl_set_adjoint, adjoint.h): the loss (AdjointLoss) with its epsilon, the detector weight
    // (nx, ny) in the detector's layout (empty: none), the data of one probe batch (adj_P, nx, ny), the waves psi_1 .. psi_nz-1 of the
    // forward loop (nz - 1, adj_P, nx, pitch) -- psi_0 is psi0 --, the float64 accumulator (nz, nx, ny), the slab of the loss
    // partials and the losses of a batch.  While adj_on the handle is on the two-pass loop (set_loop_mode); msl_adjoint_add runs
    // slice_loop with the split row step and the store between its halves
    int adj_on = ADJ_OFF, adj_P = 0;
    float adj_eps = 0.f;
    DevBuf<float> adj_w, adj_D;
    DevBuf<float2> adj_stack;
    DevBuf<double> adj_grad, adj_part, adj_loss;
    // gradients with respect to atom positions (msl_adjoint_positions): pg_valid while the sorted phase tables,
    // the order, the bin starts and the form-factor tables are those of a single-frame msl_build_potential of pg_n atoms and pg_nsp
    // species read along pg_ax1 / pg_ax2 (drop_position_tables clears it); the tile list, the images B_s of a chunk of slices (pitch
    // ny), an uploaded Gamma and the result (pg_n, 3), grown on demand
    bool pg_valid = false;
    int64_t pg_n = 0;
    int pg_nsp = 0, pg_ax1 = 0, pg_ax2 = 1;
    DevBuf<int4> pg_tiles;
    DevBuf<float2> pg_img;
    DevBuf<double> pg_gamma, pg_out;
    // gradients with respect to scan positions and aberrations (msl_adjoint_probe_params): pm_valid while the
    // probe buffer holds what msl_set_probes built at a convergent aperture (drop_probe_recipe clears it), with the recipe that call
    // used -- the aperture, the wavelength, the Cartesian coefficients (all zero without aberrations) and the positions (pm_dxy, on the device) -- so that a
    // later msl_set_aberrations or msl_set_beam cannot come between the probes and their derivative; pm_g: the images of the work
    // buffer that hold the probe gradient of the last msl_adjoint_add (0: none); the partial rows and the sums (B, PM_SLOTS), grown
    // on demand
    bool pm_valid = false;
    int pm_g = 0;
    double pm_mrad = 0.0, pm_wavelength = 0.0;
    ProbeAberrations pm_ab{};
    DevBuf<double> pm_dxy, pm_part, pm_sums;
    // frozen phonons (msl_set_structure): the base structure resident on the device -- positions (n, 3), widths, Z and the species
    // maps that stage_atoms sends per call -- with the host's copy of the maps and the axes; msl_build_thermal generates the
    // positions of any configuration from it (thermal_positions_kernel), so no per-frame array and no caller pointer is kept
    DevBuf<double> th_pos0, th_sigma;
    DevBuf<int> th_Z, th_z2s, th_species;
    int th_map_z2s[104] = {0}, th_map_species[104] = {0}, th_nsp = 0;
    int64_t th_n = 0;
    int32_t th_ax1 = 0, th_ax2 = 1, th_axs = 2;
    bool have_structure = false;
    // phonon modes (msl_set_modes) on top of the resident structure: the basis atom of every atom, q (M, 3), tau (M), W (M, nb, 3)
    // complex, and the coefficient table C (frame_batch, M) that mode_coefficients_kernel fills for every build
    DevBuf<int> md_basis;
    DevBuf<double> md_q, md_tau, md_W;
    DevBuf<double2> md_C;
    int md_M = 0, md_nb = 0;
    bool md_dynamic = true, have_modes = false;
    DevBuf<double> d_xy;
    // probe aberrations (msl_set_aberrations): (magnitude, angle) of the fourteen terms; read by every msl_set_probes
    double aberr_polar[14][2] = {};
    bool have_aberr = false;       // some magnitude is non-zero: msl_set_probes launches probe_kspace_aberr_kernel
    // counters
    msl_counters ctr{};
    double ms_kind[K_NKINDS] = {0, 0, 0};
    uint64_t n_kind[K_NKINDS] = {0, 0, 0};
    std::vector<EventSet> ring;
    int ring_pos = 0;
    EventSet* cur = nullptr;
    int lds_limit = 160 * 1024;
};

namespace {

int fail(msl_handle* h, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (h) h->err = buf; else g_create_error = buf;
    return code;
}

// Diagnostic switches (A/B runs, cross-checks of the tests) are read from the environment ONLY when MSL_DEBUG is set: a stray
// MSL_* variable in a user's environment must not change which kernels run.
const char* dbg_env(const char* name) { return getenv("MSL_DEBUG") ? getenv(name) : nullptr; }

#define HIPCHK(h, expr)                                                                              \
    do {                                                                                             \
        hipError_t _e = (expr);                                                                      \
        if (_e != hipSuccess)                                                                        \
            return fail(h, MSL_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)

bool factorize(int N, FftPlan& pl) {
    static const int cand[] = {8, 4, 2, 3, 5, 7, 11, 13};
    pl.N = N; pl.n_stages = 0;
    int n = N;
    for (int r : cand) {
        while (n % r == 0 && n > 1) {
            if (pl.n_stages >= MSL_MAX_STAGES) return false;
            pl.radix[pl.n_stages++] = r;
            n /= r;
        }
    }
    return n == 1;
}

// in-place radix-2 FFT in double on the host (Bluestein filter setup only)
void host_fft_pow2(std::vector<double>& re, std::vector<double>& im) {
    const int n = (int)re.size();
    for (int i = 1, j = 0; i < n; ++i) {
        int bit = n >> 1;
        for (; j & bit; bit >>= 1) j ^= bit;
        j ^= bit;
        if (i < j) { std::swap(re[i], re[j]); std::swap(im[i], im[j]); }
    }
    for (int len = 2; len <= n; len <<= 1) {
        for (int i = 0; i < n; i += len)
            for (int k = 0; k < len / 2; ++k) {
                const double a = -2.0 * M_PI * k / len, c = cos(a), s = sin(a);
                const int u = i + k, v = i + k + len / 2;
                const double xr = re[v] * c - im[v] * s, xi = re[v] * s + im[v] * c;
                re[v] = re[u] - xr; im[v] = im[u] - xi; re[u] += xr; im[u] += xi;
            }
    }
}

// Bluestein's chirp of n points, w[i] = exp(-i pi i^2 / n) (w holds n or more entries, the rest untouched), and its filter: the FFT of
// length M (a power of two >= 2n - 1) of the conjugate chirp wrapped to negative lags, unscaled, in (fr, fi)
void host_chirp(int n, int M, std::vector<float2>& w, std::vector<double>& fr, std::vector<double>& fi) {
    fr.assign(M, 0.0); fi.assign(M, 0.0);
    for (int i = 0; i < n; ++i) {
        const long long q = ((long long)i * i) % (2LL * n);
        const double a = -M_PI * (double)q / (double)n;
        w[i] = make_float2((float)cos(a), (float)sin(a));
        fr[i] = cos(a); fi[i] = -sin(a);
        if (i) { fr[M - i] = fr[i]; fi[M - i] = fi[i]; }
    }
    host_fft_pow2(fr, fi);
}

int make_plan(msl_handle* h, FftPlan& pl, int N) {
    if (pl.ok && pl.N == N) return MSL_OK;
    pl.ok = false;
    if (N < 1) return fail(h, MSL_ERR_INVALID, "FFT length %d", N);
    int M = N;
    bool native = factorize(N, pl);
    if (!native) {
        // Bluestein: convolution length = power of two >= 2N-1
        M = 1;
        while (M < 2 * N - 1) M <<= 1;
        FftPlan tmp;
        if (!factorize(M, tmp)) return fail(h, MSL_ERR_UNSUPPORTED, "FFT length %d: no plan", N);
        pl.n_stages = tmp.n_stages;
        for (int i = 0; i < tmp.n_stages; ++i) pl.radix[i] = tmp.radix[i];
    }
    pl.N = N; pl.M = M;
    if ((size_t)M * 8 * 2 > (size_t)h->lds_limit)
        return fail(h, MSL_ERR_UNSUPPORTED, "FFT length %d%s does not fit the LDS-resident kernel", N,
                    native ? "" : " (Bluestein, prime factor > 13)");
    std::vector<float2> tw(M);
    for (int j = 0; j < M; ++j) {
        double a = -2.0 * M_PI * (double)j / (double)M;
        tw[j] = make_float2((float)cos(a), (float)sin(a));
    }
    int rc = pl.tw.alloc(h, (size_t)M);
    if (rc) return rc;
    HIPCHK(h, hipMemcpyAsync(pl.tw, tw.data(), M * sizeof(float2), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (!native) {
        std::vector<float2> chirp(N);
        std::vector<double> br, bi;
        host_chirp(N, M, chirp, br, bi);
        std::vector<float2> bf(M);
        for (int j = 0; j < M; ++j) bf[j] = make_float2((float)(br[j] / M), (float)(bi[j] / M));
        if ((rc = pl.chirp.alloc(h, (size_t)N)) || (rc = pl.bfilt.alloc(h, (size_t)M))) return rc;
        HIPCHK(h, hipMemcpyAsync(pl.chirp, chirp.data(), N * sizeof(float2), hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(pl.bfilt, bf.data(), M * sizeof(float2), hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    pl.ok = true;
    return MSL_OK;
}

// ---- per-launch event timing -------------------------------------------------------------
int resolve_set(msl_handle* h, EventSet& s) {
    if (!s.pending) return MSL_OK;
    if (s.used >= 2) {
        HIPCHK(h, hipEventSynchronize(s.ev[s.used - 1]));
        for (int i = 0; i + 1 < s.used; ++i) {
            float ms = 0.f;
            HIPCHK(h, hipEventElapsedTime(&ms, s.ev[i], s.ev[i + 1]));
            int k = s.kind[i];
            h->ms_kind[k] += ms;
            h->n_kind[k] += 1;
        }
    }
    s.used = 0; s.pending = false;
    return MSL_OK;
}

int begin_timed(msl_handle* h, int max_launches) {
    if (!h->cfg.launch_timing) { h->cur = nullptr; return MSL_OK; }
    if (h->ring.empty()) h->ring.resize(4);
    EventSet& s = h->ring[h->ring_pos];
    h->ring_pos = (h->ring_pos + 1) % (int)h->ring.size();
    int rc = resolve_set(h, s);
    if (rc) return rc;
    while ((int)s.ev.size() < max_launches + 1) {
        hipEvent_t e;
        HIPCHK(h, hipEventCreate(&e));
        s.ev.push_back(e);
    }
    s.kind.assign(max_launches + 1, K_OTHER);
    s.used = 0;
    HIPCHK(h, hipEventRecord(s.ev[s.used++], h->stream));
    s.pending = true;
    h->cur = &s;
    return MSL_OK;
}

int mark_launch(msl_handle* h, int kind) {
    EventSet* s = h->cur;
    if (!s || s->used >= (int)s->ev.size()) return MSL_OK;
    s->kind[s->used - 1] = kind;
    HIPCHK(h, hipEventRecord(s->ev[s->used++], h->stream));
    return MSL_OK;
}

// a kernel's dynamic LDS may go up to the whole LDS of a CU (the default limit is 64 KB)
template <typename K>
void allow_lds(const msl_handle* h, K kernel) {
    (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, h->lds_limit);
}

// launch of a kernel with `lds` bytes of dynamic LDS on the handle's stream, as a timed launch of `kind`
template <typename K, typename... A>
int launch_lds(msl_handle* h, K kernel, dim3 grid, dim3 block, size_t lds, int kind, const A&... args) {
    allow_lds(h, kernel);
    hipLaunchKernelGGL(kernel, grid, block, lds, h->stream, args...);
    HIPCHK(h, hipGetLastError());
    return mark_launch(h, kind);
}

int resolve_all(msl_handle* h) {
    for (auto& s : h->ring) { int rc = resolve_set(h, s); if (rc) return rc; }
    h->cur = nullptr;
    return MSL_OK;
}

// ---- generic line-FFT launch ----------------------------------------------------------------
struct LineArgs {
    const float2* in = nullptr; float2* out = nullptr; float* out_real = nullptr;
    long long n_lines = 0; int lines_per_image = 1;
    long long in_es = 1, in_ls = 0, in_is = 0, out_es = 1, out_ls = 0, out_is = 0;
    int contiguous_lines = 0;
    int fft1 = 0, fft2 = 0;         // the common two-step form: [fft1] x m1 [fft2] store(x m2)
    int m1_kind = MUL_NONE, m2_kind = MUL_NONE; const float2* m1 = nullptr; const float2* m2 = nullptr;
    // general form (used when n_steps > 0): step i = [FFT fft[i]] then [x mul[i]]
    int n_steps = 0; int fft[MSL_GEN_STEPS] = {0, 0, 0, 0}; int mkind[MSL_GEN_STEPS] = {0, 0, 0, 0};
    const float2* mul[MSL_GEN_STEPS] = {nullptr, nullptr, nullptr, nullptr};
    int out_contiguous = -1;        // store mapping; -1 = same as contiguous_lines
    long long m1_ls = 0, m2_ls = 0;
    int store_mode = STORE_C64; int shift_n = 0, shift_r = 0; float scale = 1.f; float sigma = 0.f;
    int win_n0 = 0, win_nn = 0, win_r0 = 0, win_nr = 0;      // win_nn > 0: store only the window of the shifted output
    int group = 0; long long out_gs = 0, m_gs = 0;           // frame batching (LineJob)
};

int launch_lines(msl_handle* h, const FftPlan& pl, const LineArgs& a, int kind) {
    LineJob job{};
    job.in = a.in; job.out = a.out; job.out_real = a.out_real; job.tw = pl.tw; job.m2 = a.m2;
    job.n_lines = a.n_lines; job.in_es = a.in_es; job.in_ls = a.in_ls; job.in_is = a.in_is;
    job.out_es = a.out_es; job.out_ls = a.out_ls; job.out_is = a.out_is; job.m1_ls = a.m1_ls; job.m2_ls = a.m2_ls;
    job.N = pl.N; job.lines_per_image = a.lines_per_image; job.contiguous_lines = a.contiguous_lines;
    job.m2_kind = a.m2_kind;
    if (a.n_steps > 0) {
        job.n_steps = a.n_steps;
        for (int i = 0; i < a.n_steps; ++i) { job.fft[i] = a.fft[i]; job.mkind[i] = a.mkind[i]; job.mul[i] = a.mul[i]; }
    } else {
        job.n_steps = 2;
        job.fft[0] = a.fft1; job.mkind[0] = a.m1_kind; job.mul[0] = a.m1;
        job.fft[1] = a.fft2; job.mkind[1] = MUL_NONE; job.mul[1] = nullptr;
    }
    job.out_contiguous = a.out_contiguous < 0 ? a.contiguous_lines : a.out_contiguous;
    job.store_mode = a.store_mode; job.shift_n = a.shift_n; job.shift_r = a.shift_r;
    job.win_n0 = a.win_n0; job.win_nn = a.win_nn; job.win_r0 = a.win_r0; job.win_nr = a.win_nr;
    job.group = a.group; job.out_gs = a.out_gs; job.m_gs = a.m_gs;
    job.n_stages = pl.n_stages; for (int i = 0; i < pl.n_stages; ++i) job.radix[i] = pl.radix[i];
    job.scale = a.scale; job.sigma = a.sigma;
    const int N = pl.M;         // sizing follows the transform length (M > N for Bluestein lines)
    job.M = pl.M; job.chirp = pl.chirp; job.bfilt = pl.bfilt;
    bool has5 = false;
    for (int i = 0; i < pl.n_stages; ++i) has5 |= (pl.radix[i] == 5);
    // values per thread the plan's radices allow under either radix-5 policy (16 for powers of two, 14 with a 7, ...)
    auto elems_per_thread = [&](bool ceil5) {
        int e = MSL_GEN_E;
        for (int i = 0; i < pl.n_stages; ++i) e = std::min(e, gen_elems_per_thread(pl.radix[i], ceil5));
        return e;
    };
    int C = 1, nthreads = 64;
    size_t lds = 0;
    // tile of C lines, block size, and the resident waves per CU that result (128 VGPRs: at most 16)
    auto configure = [&](bool ceil5) -> long long {
        const int epl = elems_per_thread(ceil5);
        const int max_elems = epl * 1024;
        if (a.contiguous_lines) C = 16; else C = std::max(1, std::min(16, 8192 / N));
        C = (int)std::min<long long>(C, a.n_lines);
        job.npad = (a.contiguous_lines || job.out_contiguous) ? (N | 1) : N;      // odd pitch: conflict-free when lines are the fast index
        auto lds_need = [&](int c, bool tw) { return (size_t)MSL_GEN_HEADER + (size_t)c * job.npad * 8 + (tw ? (size_t)N * 8 : 0); };
        while (C > 1 && ((long long)C * N > max_elems || lds_need(C, false) > (size_t)h->lds_limit)) C >>= 1;
        if ((long long)C * N > max_elems || lds_need(C, false) > (size_t)h->lds_limit) return -1;
        job.C = C;
        job.tw_in_lds = lds_need(C, true) <= (size_t)h->lds_limit ? 1 : 0;
        lds = lds_need(C, job.tw_in_lds != 0);
        nthreads = (int)(((long long)C * N + epl - 1) / epl);
        nthreads = std::min(1024, std::max(64, (nthreads + 63) / 64 * 64));
        const int waves = nthreads / 64;
        const long long wgs = std::min<long long>((long long)(h->lds_limit / lds), 16 / waves);
        return std::max<long long>(1, wgs) * waves;              // resident waves per CU
    };
    bool ceil5 = false;
    long long score = configure(false);
    if (has5) {
        const long long score5 = configure(true);
        if (score5 > score) ceil5 = true; else score = configure(false);
    }
    if (score < 0) return fail(h, MSL_ERR_UNSUPPORTED, "line length %d too long for the LDS kernel", pl.N);
    long long tiles = (a.n_lines + C - 1) / C;
    if (tiles > 0x7fffffffLL) return fail(h, MSL_ERR_UNSUPPORTED, "too many FFT tiles");
    int rset = 0;
    for (int i = 0; i < pl.n_stages; ++i) {
        if (pl.radix[i] == 3 || pl.radix[i] == 5 || pl.radix[i] == 7) rset = std::max(rset, 1);
        if (pl.radix[i] > 8) rset = 2;
    }
    const dim3 grid((unsigned)tiles), block(nthreads);
    if (rset == 0) hipLaunchKernelGGL((line_fft_kernel<0, false>), grid, block, lds, h->stream, job);
    else if (rset == 1 && !ceil5) hipLaunchKernelGGL((line_fft_kernel<1, false>), grid, block, lds, h->stream, job);
    else if (rset == 1) hipLaunchKernelGGL((line_fft_kernel<1, true>), grid, block, lds, h->stream, job);
    else if (!ceil5) hipLaunchKernelGGL((line_fft_kernel<2, false>), grid, block, lds, h->stream, job);
    else hipLaunchKernelGGL((line_fft_kernel<2, true>), grid, block, lds, h->stream, job);
    HIPCHK(h, hipGetLastError());
    return mark_launch(h, kind);
}

// row pass over (images x nx) rows of length ny; column pass over (images x ny) columns of length nx
LineArgs row_args(const msl_handle* h, const float2* in, float2* out, int images, int pitch) {
    LineArgs a;
    a.in = in; a.out = out;
    a.n_lines = (long long)images * h->cfg.nx; a.lines_per_image = h->cfg.nx;
    a.in_es = a.out_es = 1; a.in_ls = a.out_ls = pitch; a.in_is = a.out_is = (long long)h->cfg.nx * pitch;
    a.contiguous_lines = 0;
    return a;
}
LineArgs col_args(const msl_handle* h, const float2* in, float2* out, int images, int in_pitch, int out_pitch) {
    LineArgs a;
    a.in = in; a.out = out;
    a.n_lines = (long long)images * h->cfg.ny; a.lines_per_image = h->cfg.ny;
    a.in_es = in_pitch; a.out_es = out_pitch; a.in_ls = a.out_ls = 1;
    a.in_is = (long long)h->cfg.nx * in_pitch; a.out_is = (long long)h->cfg.nx * out_pitch;
    a.contiguous_lines = 1;
    return a;
}

// Timing bracket of one call: end() waits for the stream and adds the device time since begin() to *ms_total; without begin() it does
// nothing (the call only queued work).  The events are destroyed on every exit path.
struct EventPair {
    hipEvent_t a = nullptr, b = nullptr;
    ~EventPair() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
    int begin(msl_handle* h) {
        HIPCHK(h, hipEventCreate(&a)); HIPCHK(h, hipEventCreate(&b));
        HIPCHK(h, hipEventRecord(a, h->stream));
        return MSL_OK;
    }
    int end(msl_handle* h, double* ms_total) {
        if (!b) return MSL_OK;
        HIPCHK(h, hipEventRecord(b, h->stream));
        HIPCHK(h, hipEventSynchronize(b));
        float ms = 0.f;
        HIPCHK(h, hipEventElapsedTime(&ms, a, b));
        *ms_total += ms;
        return MSL_OK;
    }
};

// Probes per work item of the chunked kernels (a work item = 16 lines x a chunk of probes that share the t_k lines in
// registers; the grid is `slots` persistent workgroups).  The time of a launch is (rounds of work items over the slots) x
// (iterations per item): take the chunk that minimises it, the larger one on ties (fewer t_k loads).  Halving until every slot
// has an item, as round 1 did, wastes up to half a launch when the item count lands just above a multiple of the slots
// (300 lines x 64 probes: 304 items of 4 probes = 8 iteration times, 247 items of 5 probes = 5).
int choose_pchunk(long long line_blocks, int n_images, long long slots, int t_group) {
    int best = 1;
    long long best_cost = -1;
    for (int pc = 1; pc <= n_images; ++pc) {
        if (t_group > 0 && t_group % pc) continue;            // frame batching: a chunk stays inside one frame
        const long long items = line_blocks * ((n_images + pc - 1) / pc);
        const long long cost = ((items + slots - 1) / slots) * pc;
        if (best_cost < 0 || cost <= best_cost) { best = pc; best_cost = cost; }
    }
    return best;
}

// Persistent grid of a chunked row kernel over `line_blocks` work items per image chunk on `slots` workgroups: sets job.pchunk
// (choose_pchunk, or the MSL_ROW_PCHUNK override kept inside one frame) and returns the grid
template <typename Job>
int chunked_grid(const msl_handle* h, Job& job, long long line_blocks, long long slots) {
    int pc = choose_pchunk(line_blocks, job.n_images, slots, job.t_group);
    if (h->row_pchunk > 0) { pc = std::min(h->row_pchunk, job.n_images); if (job.t_group > 0) while (job.t_group % pc) --pc; }
    job.pchunk = pc;
    const long long items = line_blocks * ((job.n_images + pc - 1) / pc);
    return (int)std::min<long long>(items, slots);
}

// frame batching: the images of a launch are frame-of-batch * n_probes + probe, each frame with its own transmission stack
template <typename Job>
void set_frame_groups(const msl_handle* h, Job& j, int groups) {
    const msl_config& c = h->cfg;
    if (groups > 1) { j.t_group = c.n_probes; j.t_magic = (unsigned)((1ull << 32) / (unsigned)c.n_probes + 1); j.t_stride = (long long)c.nz * c.nx * c.ny; }
}

// counters after a slice loop of P images: `bytes` per pixel and slice-step, plus the transmission reads and the fused epilogue
void count_slice_loop(msl_handle* h, int P, int groups, bool fused, uint64_t bytes) {
    const msl_config& c = h->cfg;
    const size_t npix = (size_t)c.nx * c.ny;
    h->cur = nullptr;
    h->ctr.slice_steps += (uint64_t)P * c.nz;
    h->ctr.frames += groups;
    h->ctr.algorithmic_bytes += (uint64_t)P * c.nz * bytes * npix + (uint64_t)groups * c.nz * 8ull * npix + (fused ? (uint64_t)P * 16ull * npix : 0ull);
}

// ---- four-step fast path ------------------------------------------------------------------------
int fast_radix(int n) { return n == 1024 ? 32 : (n == 256 ? 16 : 0); }

// ---- host tables -------------------------------------------------------------------------------------
// copy a host table into the device buffer dst (allocated by the caller)
int copy_table(msl_handle* h, float2* dst, const std::vector<float2>& v) {
    HIPCHK(h, hipMemcpyAsync(dst, v.data(), v.size() * sizeof(float2), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return MSL_OK;
}

// a host table in a device buffer of its own
int upload(msl_handle* h, DevBuf<float2>& dst, const std::vector<float2>& v) {
    int rc = dst.alloc(h, v.size());
    return rc ? rc : copy_table(h, dst, v);
}

// twiddles of the four-step R^2-point FFT: t[k1*R + n2] = W_{R^2}^{k1 n2}
int make_tw4(msl_handle* h, DevBuf<float2>& dst, int R) {
    const int N = R * R;
    std::vector<float2> t(N);
    for (int k1 = 0; k1 < R; ++k1)
        for (int n2 = 0; n2 < R; ++n2) {
            double a = -2.0 * M_PI * (double)((k1 * n2) % N) / (double)N;
            t[k1 * R + n2] = make_float2((float)cos(a), (float)sin(a));
        }
    return upload(h, dst, t);
}

// tables of the wave-per-line 2048-point FFT: T[k1*64+n2] = W_2048^{k1 n2}, and W_64 (even lane of a pair: no twiddle; odd lane: W_64^m)
int make_wave2k_tables(msl_handle* h, DevBuf<float2>& tw, DevBuf<float2>& tw2) {
    constexpr int M = 2048;
    std::vector<float2> T(M), W(64);
    for (int k1 = 0; k1 < 32; ++k1)
        for (int n2 = 0; n2 < 64; ++n2) {
            const double a = -2.0 * M_PI * (double)(k1 * n2) / (double)M;
            T[k1 * 64 + n2] = make_float2((float)cos(a), (float)sin(a));
        }
    for (int m = 0; m < 32; ++m) {
        const double a = -2.0 * M_PI * m / 64.0;
        W[m] = make_float2(1.f, 0.f);
        W[32 + m] = make_float2((float)cos(a), (float)sin(a));
    }
    int rc = upload(h, tw, T);
    return rc ? rc : upload(h, tw2, W);
}

// chirp-z tables of n points (CzTables): M = 256 up to 128 points, 1024 up to 512, else the 2048-point wave FFT
int make_cz_tables(msl_handle* h, CzTables& o, int n) {
    const bool wave = n > 512;
    const int R = wave ? 32 : (n <= 128 ? 16 : 32), M = wave ? 2048 : R * R, NH = M / 2;
    int r = wave ? make_wave2k_tables(h, o.tw, o.tw2) : make_tw4(h, o.tw, R);
    if (r) return r;
    std::vector<float2> bw(NH, make_float2(0.f, 0.f)), bf(NH + 2, make_float2(0.f, 0.f));
    std::vector<double> cr, ci;
    host_chirp(n, M, bw, cr, ci);
    for (int j = 0; j <= NH; ++j) bf[j] = make_float2((float)(cr[j] / M), (float)(ci[j] / M));
    if ((r = upload(h, o.bw, bw)) || (r = upload(h, o.bf, bf))) return r;
    o.R = wave ? 64 : R;
    return MSL_OK;
}

template <int R>
int launch_row_fast_r(msl_handle* h, const RowJob& job, int kind) {
    constexpr int N = R * R, G = 256 / R;
    const size_t lds = (size_t)N * 16 + (size_t)G * R * (R + 1) * 4;
    const int per_cu = std::max(1, std::min(2, (int)((size_t)h->lds_limit / lds)));
    const long long slots = (long long)h->n_cus * per_cu;
    // probes per work item: as many as possible (t_z reuse) while still giving every slot an item
    RowJob j2 = job;
    const long long xg = job.nx / G;
    int pc = job.n_images;
    while (pc > 1 && xg * ((job.n_images + pc - 1) / pc) < slots) pc = (pc + 1) / 2;
    if (h->row_pchunk > 0) pc = std::min(h->row_pchunk, job.n_images);
    if (job.t_group > 0) while (job.t_group % pc) --pc;          // a chunk of probes shares one t_k line: stay inside a frame
    j2.pchunk = pc;
    const long long items = xg * ((job.n_images + pc - 1) / pc);
    const int grid = (int)std::min<long long>(items, slots);
    hipLaunchKernelGGL(row_pass_pf_kernel<R>, dim3(grid), dim3(256), lds, h->stream, j2);
    HIPCHK(h, hipGetLastError());
    return mark_launch(h, kind);
}

// HERM: column pass of the potential build on the rows kx <= nx/2 of a Hermitian spectrum
template <int R, bool HERM = false>
int launch_col_fast_r(msl_handle* h, const ColJob& job, int kind) {
    constexpr int N = R * R, CS = R * (R + 1) + 1;
    const size_t lds = ((size_t)2 * N + (size_t)16 * CS) * 8;
    const long long tiles = (long long)(job.ny / 16) * job.n_images;
    const int per_cu = std::max(1, (int)((size_t)h->lds_limit / lds));
    const int grid = (int)std::min<long long>(tiles, (long long)h->n_cus * std::min(per_cu, 2));
    if (HERM) return launch_lds(h, col_pass_kernel<R, 16, true>, dim3(grid), dim3(16 * R), lds, kind, job);
    hipLaunchKernelGGL(col_pass_kernel<R>, dim3(grid), dim3(16 * R), lds, h->stream, job);
    HIPCHK(h, hipGetLastError());
    return mark_launch(h, kind);
}
int launch_col_herm(msl_handle* h, const ColJob& job, int kind) {
    return h->Rx == 32 ? launch_col_fast_r<32, true>(h, job, kind) : launch_col_fast_r<16, true>(h, job, kind);
}

int launch_row_fast(msl_handle* h, const RowJob& job, int kind) {
    return h->Ry == 32 ? launch_row_fast_r<32>(h, job, kind) : launch_row_fast_r<16>(h, job, kind);
}
int launch_col_fast(msl_handle* h, const ColJob& job, int kind) {
    return h->Rx == 32 ? launch_col_fast_r<32>(h, job, kind) : launch_col_fast_r<16>(h, job, kind);
}

RowJob row_job(const msl_handle* h, float2* buf, int images, int pitch) {
    RowJob j{};
    j.psi = buf; j.trans = nullptr; j.py = nullptr; j.tw = h->tw4_y;
    j.image_stride = (long long)h->cfg.nx * pitch; j.pitch = pitch; j.nx = h->cfg.nx; j.n_images = images;
    return j;
}
ColJob col_job(const msl_handle* h, const float2* in, float2* out, int images, int in_pitch, int out_pitch) {
    ColJob j{};
    j.in = in; j.out = out; j.px = nullptr; j.tw = h->tw4_x;
    j.in_image_stride = (long long)h->cfg.nx * in_pitch; j.out_image_stride = (long long)h->cfg.nx * out_pitch;
    j.in_pitch = in_pitch; j.out_pitch = out_pitch; j.ny = h->cfg.ny; j.n_images = images; j.flags = 0; j.scale = 1.f;
    return j;
}

int fft2_inplace(msl_handle* h, float2* buf, int images, int dir, float scale, int pitch) {
    int rc;
    if (h->Ry) {
        RowJob r = row_job(h, buf, images, pitch);
        r.do_ifft = dir < 0; r.do_fft = dir > 0;
        if ((rc = launch_row_fast(h, r, K_OTHER))) return rc;
    } else {
        LineArgs r = row_args(h, buf, buf, images, pitch);
        r.fft1 = dir;
        if ((rc = launch_lines(h, h->plan_y, r, K_OTHER))) return rc;
    }
    if (h->Rx) {
        ColJob c = col_job(h, buf, buf, images, pitch, pitch);
        c.flags = dir > 0 ? COL_FWD : COL_INV; c.scale = scale;
        return launch_col_fast(h, c, K_OTHER);
    }
    LineArgs c = col_args(h, buf, buf, images, pitch, pitch);
    c.fft1 = dir; c.scale = scale;
    return launch_lines(h, h->plan_x, c, K_OTHER);
}

// Exit-wave epilogue, second half: FFT along x of the y-transformed exit waves in psi, fftshift of both axes and
// scatter into slot `slot` of the (P, T_local, wx, wy) result (calculators.py:284-290).  With a k-window only the
// columns inside it are transformed and only the rows inside it are stored.
// staged full-resolution windows of `groups` frames x P probes -> binned frame slots slot .. slot+groups-1
int bin_frames(msl_handle* h, int slot, int groups, float2* result) {
    const msl_config& c = h->cfg;
    const long long total = (long long)h->wpix * c.n_probes * groups;
    hipLaunchKernelGGL(bin_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->stream, h->bin_stage, result, c.n_probes, groups,
                       c.n_frames, slot, h->wx, h->wy, h->bx, h->by, (long long)h->wpitch);
    HIPCHK(h, hipGetLastError());
    return mark_launch(h, K_OTHER);
}

// src: y-transformed waves in psi's layout (default psi); result: (P, T_local, wpitch) block (default wf); px: weight of the x
// frequencies after the FFT (the layer tap), or null
int epilogue_x_pass(msl_handle* h, int slot, int groups = 1, const float2* src = nullptr, float2* result = nullptr, const float2* px = nullptr) {
    const msl_config& c = h->cfg;
    if (!src) src = h->psi;
    if (!result) result = h->wf;
    const int P = c.n_probes * groups;               // image = frame-of-batch * n_probes + probe -> wf[probe][slot + frame]
    const bool binned = h->bin_stage != nullptr;
    // binning: the full-resolution window of every image goes to the staging buffer (image-major), bin_kernel sums it
    // into the frame slots -- 16 B/pixel/(probe, frame) extra against 16 B/pixel/slice-step of the loop
    float2* dst = binned ? h->bin_stage : result + (size_t)slot * h->wpitch;
    const long long out_is = binned ? (long long)h->wx * h->wy : (long long)c.n_frames * h->wpitch;
    const int og = binned ? 1 : groups;               // staged images stay image-major; bin_kernel regroups them by frame
    const bool windowed = (h->wx != c.nx) || (h->wy != c.ny);
    // the shifted scatter moves whole tiles of 16 columns by ny/2: ny % 32 == 16 would put half of one tile past the end of the rows
    const bool fast_ok = h->Rx && c.ny % 32 == 0 && (!windowed || h->wy % 32 == 0);
    if (fast_ok) {
        ColJob k = col_job(h, src, dst, P, h->pitch, h->wy);
        k.flags = COL_FWD | COL_SHIFT; k.out_image_stride = out_is;
        if (px) { k.px = px; k.flags |= COL_MULPX; }
        if (og > 1) { k.out_group = c.n_probes; k.out_group_stride = (long long)h->wpitch; }
        if (windowed) { k.win_c0 = h->wy0; k.win_nc = h->wy; k.win_x0 = h->wx0; k.win_nx = h->wx; }
        int rc = launch_col_fast(h, k, K_OTHER);
        return (rc || !binned) ? rc : bin_frames(h, slot, groups, result);
    }
    LineArgs k = col_args(h, src, dst, P, h->pitch, h->wy);
    k.fft1 = +1;
    if (px) { k.m1_kind = MUL_VEC; k.m1 = px; }
    k.out_is = out_is;
    if (og > 1) { k.group = c.n_probes; k.out_gs = (long long)h->wpitch; }
    k.shift_n = c.nx / 2; k.shift_r = c.ny / 2;
    if (windowed) { k.win_n0 = h->wx0; k.win_nn = h->wx; k.win_r0 = h->wy0; k.win_nr = h->wy; }
    int rc = launch_lines(h, h->plan_x, k, K_OTHER);
    return (rc || !binned) ? rc : bin_frames(h, slot, groups, result);
}

// ---- thickness series: the layer tap ---------------------------------------
// After the pass that applied t_k the work buffer holds, in the layout that pass wrote,
//   one-pass loops:  S = A_d psi_k  (A_d = ifft_d P_d fft_d, d = the pass's axis)   ->  fft2(psi_k) = conj(P_d)[k_d] fft2(S)
//   two-pass loop:   S = (P_y / ny) fft_y psi_k                                      ->  fft_y(psi_k) = ny conj(P_y)[k_y] S
// The tap copies S into natural order (layer_tap_gather_kernel; the two-pass loop's weight applied there), transforms along y (with
// conj(P_y) when d = y), and runs the exit epilogue into block `layer_block[k]` (with conj(P_x) after the x-FFT when d = x).
// The passes of the loop are untouched.  axis: 0 = the pass ran along y, 1 = along x, 2 = two-pass loop.
constexpr int TAP_MAX_LAUNCHES = 4;                  // gather, row FFT, column epilogue, binning
constexpr int LR_MAX_LAUNCHES = 4;                   // layer reductions: detector tiles, their finish, polar bins, patterns

int n_taps(const msl_handle* h) { return (int)h->layer_slices.size(); }

// blocks of the resident result: the reduce mode taps into a block of its own and keeps the exit block only
int n_result_layers(const msl_handle* h) { return h->lr_on ? 1 : n_taps(h) + 1; }

// timed launches the taps add to a fused slice loop; in the reduce mode also the reductions of every layer and of the exit
int tap_launches(const msl_handle* h) {
    return TAP_MAX_LAUNCHES * n_taps(h) + (h->lr_on ? LR_MAX_LAUNCHES * (n_taps(h) + 1) : 0);
}

// the reductions of layer l over the frame slots [slot, slot + count) of `block`, queued on the stream (defined with the reductions)
int layer_reduce_queue(msl_handle* h, int l, const float2* block, int slot, int count);

size_t layer_block_elems(const msl_handle* h) { return h->wpitch * (size_t)h->cfg.n_probes * h->cfg.n_frames; }

int layer_tap(msl_handle* h, int k, int slot, int groups, const float2* buf, bool transposed, int order, int rp, int axis) {
    if (slot < 0 || h->layer_block.empty() || h->layer_block[k] < 0) return MSL_OK;
    const msl_config& c = h->cfg;
    const int P = c.n_probes * groups;
    TapGatherJob g{};
    g.src = buf; g.dst = h->tap;
    g.wy = axis == 2 ? h->tap_cy : nullptr; g.wscale = (float)c.ny;
    g.src_is = transposed ? (long long)c.ny * h->pitchT : (long long)c.nx * h->pitch;
    g.dst_is = (long long)c.nx * h->pitch;
    g.src_pitch = transposed ? h->pitchT : h->pitch; g.dst_pitch = h->pitch;
    g.nx = c.nx; g.ny = c.ny; g.transposed = transposed ? 1 : 0; g.order = order; g.rp = rp;
    const int n_lines = transposed ? c.ny : c.nx, len = transposed ? c.nx : c.ny;
    hipLaunchKernelGGL((layer_tap_gather_kernel<32, 64>), dim3((len + 63) / 64, (n_lines + 31) / 32, P), dim3(256), 0, h->stream, g);
    HIPCHK(h, hipGetLastError());
    int rc = mark_launch(h, K_OTHER);
    if (rc) return rc;
    if (axis != 2) {
        if (h->Ry) {
            RowJob r = row_job(h, h->tap, P, h->pitch);
            r.do_fft = true; r.py = axis == 0 ? h->tap_cy : nullptr;
            rc = launch_row_fast(h, r, K_OTHER);
        } else {
            LineArgs r = row_args(h, h->tap, h->tap, P, h->pitch);
            r.fft1 = +1;
            if (axis == 0) { r.m1_kind = MUL_VEC; r.m1 = h->tap_cy; }
            rc = launch_lines(h, h->plan_y, r, K_OTHER);
        }
        if (rc) return rc;
    }
    float2* dst = h->lr_on ? h->lr_block.p : h->layers + (size_t)h->layer_block[k] * layer_block_elems(h);
    if ((rc = epilogue_x_pass(h, slot, groups, h->tap, dst, axis == 1 ? h->tap_cx : nullptr)))
        return rc;
    // read S, write + read the copy (twice with the row FFT), write the layer's spectra
    const uint64_t img = (uint64_t)c.nx * c.ny * 8ull;
    h->ctr.algorithmic_bytes += (uint64_t)P * (img * (axis == 2 ? 3 : 5) + (uint64_t)h->wpix * 8ull);
    return MSL_OK;
}

// what a fused slice loop does after the pass of slice k: the tap, and in the reduce mode the layer's reductions right behind it --
// stream order lets the next tap overwrite the block
int tap_step(msl_handle* h, int k, int slot, int groups, const float2* buf, bool transposed, int order, int rp, int axis) {
    int rc = layer_tap(h, k, slot, groups, buf, transposed, order, rp, axis);
    if (rc || !h->lr_on || slot < 0 || h->layer_block[k] < 0) return rc;
    return layer_reduce_queue(h, h->layer_block[k], h->lr_block, slot, groups);
}

// only the 256 / 512 / 1024-point kernels read and write the interleaved line order (16-byte loads in the reader) between two passes
bool interleaves(const msl_handle::OpDir& o) { return o.kind == AX_FOURSTEP || o.kind == AX_TWO; }

// line order of the output of a transposing pass of direction `o` launched with `flags` / `perm_shift` (launch_rowT_dir)
int tap_order(const msl_handle::OpDir& o, int flags, int perm_shift, int* rp) {
    *rp = 8 << perm_shift;
    if (!(flags & P2_OUT_PAIRED)) return TAP_NATURAL;
    if (o.kind == AX_WAVE2K) return TAP_PAIRED;
    return interleaves(o) ? TAP_INTERLEAVED : TAP_NATURAL;
}

// ---- one-pass-per-slice path ------------------------------------------------------------------------
// psi0 (P, nx, pitch) -> psi0T (P, ny, pitchT): needed when the first pass of the slice loop runs along x
int transpose_probes(msl_handle* h) {
    const msl_config& c = h->cfg;
    // frame batching: every frame of a batch starts from the same probes -- one copy per frame
    const size_t group = (size_t)c.n_probes * c.nx * h->pitch;
    for (int f = 1; f < h->FB; ++f)
        HIPCHK(h, hipMemcpyAsync(h->psi0 + f * group, h->psi0, group * sizeof(float2), hipMemcpyDeviceToDevice, h->stream));
    if (!h->onepass_planned || !h->need_psi0T) return MSL_OK;       // the first pass runs along y, on layout A
    dim3 grid((c.ny + 31) / 32, (c.nx + 31) / 32, c.n_probes * h->FB);
    hipLaunchKernelGGL(transpose_kernel, grid, dim3(256), 0, h->stream, h->psi0, h->psi0T, c.nx, c.ny, h->pitch, h->pitchT,
                       (long long)c.nx * h->pitch, (long long)c.ny * h->pitchT);
    HIPCHK(h, hipGetLastError());
    return MSL_OK;
}

// slice s is used by a pass along x (needs t transposed) iff its distance to the last slice is odd
inline bool slice_is_transposed(const msl_handle* h, int s) {
    if (!h->onepass) return false;
    return h->scheme_b ? ((s & 1) != 0) : (((h->cfg.nz - 1 - s) & 1) != 0);
}

// natural t (nz,nx,ny) of the stack in batch slot `slot` -> transposed copies of the odd-distance slices in transT (upload / set_beam paths)
int transpose_odd_slices(msl_handle* h, int slot) {
    if (!h->onepass) return MSL_OK;
    const msl_config& c = h->cfg;
    const size_t npix = (size_t)c.nx * c.ny;
    // the transposed slices are every second one: a single launch with the slice index on grid.z
    const int first = slice_is_transposed(h, 0) ? 0 : 1;
    const int count = (c.nz - first + 1) / 2;
    for (int z0 = 0; z0 < count; z0 += 65535) {
        const int nzb = std::min(65535, count - z0);
        dim3 grid((c.ny + 31) / 32, (c.nx + 31) / 32, nzb);
        const size_t off = (size_t)slot * c.nz * npix + (size_t)(first + 2 * z0) * npix;
        hipLaunchKernelGGL(transpose_kernel, grid, dim3(256), 0, h->stream, h->trans + off, h->transT + off, c.nx, c.ny,
                           c.ny, c.nx, (long long)(2 * npix), (long long)(2 * npix));
    }
    HIPCHK(h, hipGetLastError());
    return MSL_OK;
}

// the reverse: the natural copies of the slices the one-pass loop keeps transposed, transT -> trans, of the stack in batch slot `slot`
int restore_natural_slices(msl_handle* h, int slot) {
    if (!h->onepass) return MSL_OK;
    const msl_config& c = h->cfg;
    const size_t npix = (size_t)c.nx * c.ny;
    const int first = slice_is_transposed(h, 0) ? 0 : 1;
    const int count = (c.nz - first + 1) / 2;
    for (int z0 = 0; z0 < count; z0 += 65535) {
        const int nzb = std::min(65535, count - z0);
        dim3 grid((c.nx + 31) / 32, (c.ny + 31) / 32, nzb);
        const size_t off = (size_t)slot * c.nz * npix + (size_t)(first + 2 * z0) * npix;
        hipLaunchKernelGGL(transpose_kernel, grid, dim3(256), 0, h->stream, h->transT + off, h->trans + off, c.ny, c.nx, c.nx, c.ny,
                           (long long)(2 * npix), (long long)(2 * npix));
    }
    HIPCHK(h, hipGetLastError());
    return MSL_OK;
}

// transposing pass on R^2-point lines (1024 / 256), rowt_pass.h; the kernels live in slice_pass.hip
template <int R>
int launch_rowT_r(msl_handle* h, RowTJob job, int kind) {
    constexpr int LINES = 16;
    const size_t lds = rowT_lds_bytes(R);
    // R = 32: ~235 VGPRs, 152 KB -> one workgroup per CU; R = 16: 138 VGPRs, 41 KB -> three
    const int cap = (R == 16) ? 3 : 2;
    const int per_cu = std::max(1, std::min(cap, (int)((size_t)h->lds_limit / lds)));
    const int grid = chunked_grid(h, job, job.n_lines / LINES, (long long)h->n_cus * per_cu);
    if (!rowT_launch(R, job, grid, (size_t)h->lds_limit, h->stream)) return fail(h, MSL_ERR_STATE, "transposing pass: no kernel for flags %d", job.flags);
    HIPCHK(h, hipGetLastError());
    return mark_launch(h, kind);
}

// A runtime value as a template argument: f(std::bool_constant<v>{}), and f(std::integral_constant<int, V>{}) for the V of the
// list that equals v (the last of the list when none does, as the else of the ladder this replaces).  f is a generic lambda that
// reads the value back with decltype(arg)::value, so a kernel's argument list is written once for all its instantiations.
template <typename F>
auto with_bool(bool v, F&& f) {
    return v ? f(std::true_type{}) : f(std::false_type{});
}
template <int V0, int... Vs, typename F>
auto with_int(int v, F&& f) {
    if constexpr (sizeof...(Vs) == 0) return f(std::integral_constant<int, V0>{});
    else return v == V0 ? f(std::integral_constant<int, V0>{}) : with_int<Vs...>(v, f);
}

// the paired-lines flags of a job as the template arguments <IN_P, OUT_P> of `launch`
template <typename F>
int paired_dispatch(const RowTJob& job, F&& launch) {
    return with_bool(job.flags & P2_IN_PAIRED, [&](auto in_p) { return with_bool(job.flags & P2_OUT_PAIRED, [&](auto out_p) { return launch(in_p, out_p); }); });
}

// lines of 2 R^2 = 512 points
template <bool IN_P, bool OUT_P>
int launch_rowT2_io(msl_handle* h, RowTJob job, int kind) {
    constexpr int R = 16;
    const size_t lds = rowT2_lds_bytes(R);
    const int per_cu = std::max(1, std::min(2, (int)((size_t)h->lds_limit / lds)));
    const int grid = chunked_grid(h, job, job.n_lines / 16, (long long)h->n_cus * per_cu);
    return launch_lds(h, rowT2_pass_kernel<R, IN_P, OUT_P>, dim3(grid), dim3(16 * R), lds, kind, job);
}

// lines of any length <= R^2/2: zero-padded cyclic convolution on the register FFTs
template <int R>
int launch_rowTB_r(msl_handle* h, RowTJob job, int kind) {
    const size_t lds = rowTB_lds_bytes(R);
    const int per_cu = std::max(1, std::min(R == 16 ? 4 : 1, (int)((size_t)h->lds_limit / lds)));
    const int grid = chunked_grid(h, job, (job.n_lines + 15) / 16, (long long)h->n_cus * per_cu);
    return launch_lds(h, rowTB_pass_kernel<R>, dim3(grid), dim3(16 * R), lds, kind, job);
}

// lines of 513..1024 points: the same convolution on the wave-per-line 2048-point register FFT
template <bool IN_P, bool OUT_P>
int launch_rowTB2_io(msl_handle* h, RowTJob job, int kind) {
    const int grid = chunked_grid(h, job, (job.n_lines + 7) / 8, h->n_cus);
    return launch_lds(h, rowTB2_pass_kernel<IN_P, OUT_P>, dim3(grid), dim3(512), rowTB2_lds_bytes(), kind, job);
}

// 2048-point lines, one wave per line (fft2048_wave)
template <bool IN_P, bool OUT_P>
int launch_rowTW_io(msl_handle* h, RowTJob job, int kind) {
    const int grid = chunked_grid(h, job, job.n_lines / 8, h->n_cus);
    return launch_lds(h, rowTW_pass_kernel<IN_P, OUT_P>, dim3(grid), dim3(512), rowTW_lds_bytes(), kind, job);
}

// lines of a smooth length A * B (A, B <= 32; G = 16 / 32 lanes per line) or 2 A * B (G = 64: one wave per line, tiles of 8 lines):
// direct mixed-radix transform (rowtm_pass.h)
int launch_rowTM(msl_handle* h, const msl_handle::OpDir& o, RowTJob job, int kind) {
    const int n = o.n;
    int A = 0, B = 0, G = 0;
    if (!rowTM_factors(n, &A, &B, &G)) return fail(h, MSL_ERR_STATE, "mixed-radix pass: no kernel for %d points", n);
    const size_t lds = G == 64 ? rowTM2_lds_bytes(A, B) : rowTM_lds_bytes(A, B);
    if (lds > (size_t)h->lds_limit) return fail(h, MSL_ERR_STATE, "mixed-radix pass: %zu bytes of LDS for %d points", lds, n);
    // ~230 VGPRs: two waves per SIMD, i.e. one workgroup of 512 threads or two of 256 per CU
    const int per_cu = std::max(1, std::min(G == 16 ? 2 : 1, (int)((size_t)h->lds_limit / lds)));
    const int lines = G == 64 ? 8 : 16;
    const int grid = chunked_grid(h, job, (job.n_lines + lines - 1) / lines, (long long)h->n_cus * per_cu);
    job.tw = o.mtw;
    if (!rowTM_launch(n, job, grid, (size_t)h->lds_limit, h->stream)) return fail(h, MSL_ERR_STATE, "mixed-radix pass: no kernel for %d points", n);
    HIPCHK(h, hipGetLastError());
    return mark_launch(h, kind);
}

// one transposing pass along direction `o`: the kernel of its kind, running the program (fft, x P, ifft, x t, fft, x P, ifft)
// with a transposing store
int launch_rowT_dir(msl_handle* h, const msl_handle::OpDir& o, RowTJob job, int kind) {
    if (!interleaves(o) && o.kind != AX_WAVE2K) job.flags &= ~(P2_IN_PAIRED | P2_OUT_PAIRED);
    switch (o.kind) {
    case AX_MIXED:
        return launch_rowTM(h, o, job, kind);
    case AX_GENERIC: {
        const FftPlan& pl = (&o == &h->opx) ? h->plan_x : h->plan_y;
        LineArgs a;
        a.in = job.in; a.out = job.out;
        a.n_lines = (long long)job.n_images * job.n_lines; a.lines_per_image = job.n_lines;
        a.in_es = 1; a.in_ls = job.in_pitch; a.in_is = job.in_image_stride;
        a.out_es = job.out_pitch; a.out_ls = 1; a.out_is = job.out_image_stride;
        a.contiguous_lines = 0; a.out_contiguous = 1;
        a.m1_ls = pl.N;
        if (job.t_group > 0) { a.group = job.t_group; a.m_gs = job.t_stride; a.out_gs = (long long)job.t_group * job.out_image_stride; }
        int n = 0;
        if (job.flags & P2_PRE_A) {
            a.fft[n] = +1; a.mkind[n] = MUL_VEC; a.mul[n] = job.pl; ++n;
            a.fft[n] = -1; a.mkind[n] = MUL_ARRAY; a.mul[n] = job.trans; ++n;
        } else {
            a.fft[n] = 0; a.mkind[n] = MUL_ARRAY; a.mul[n] = job.trans; ++n;
        }
        if (job.flags & P2_POST_A) {
            a.fft[n] = +1; a.mkind[n] = MUL_VEC; a.mul[n] = job.pl; ++n;
            a.fft[n] = -1; a.mkind[n] = MUL_NONE; a.mul[n] = nullptr; ++n;
        }
        a.n_steps = n;
        return launch_lines(h, pl, a, kind);
    }
    case AX_WAVE2K:
        job.tw = o.tw; job.tw2 = o.tw2;
        return paired_dispatch(job, [&](auto in_p, auto out_p) { return launch_rowTW_io<decltype(in_p)::value, decltype(out_p)::value>(h, job, kind); });
    case AX_CONV4K: {                       // 1025 .. 2047 points: cyclic convolution of length 4096, two waves per line
        job.n_line = o.n;
        job.tw = o.tw; job.tw2 = o.tw2; job.bf = o.qf; job.bw = o.bw; job.pl = nullptr;
        job.pchunk = 1;
        const long long items2 = (long long)((job.n_lines + 3) / 4) * job.n_images;
        const int grid2 = (int)std::min<long long>(items2, (long long)h->n_cus);
        return launch_lds(h, rowTC2_pass_kernel, dim3(grid2), dim3(512), rowTC2_lds_bytes(), kind, job);
    }
    case AX_CONV:                           // A as one cyclic convolution of length M (two FFTs); bf = its filter
    case AX_CONV2K:
        job.n_line = o.n;
        job.tw = o.cz.tw; job.pl = nullptr; job.bf = o.qf; job.bw = nullptr;
        if (o.kind == AX_CONV2K) { job.tw2 = o.cz.tw2; return launch_rowTB2_io<false, false>(h, job, kind); }
        return o.R == 32 ? launch_rowTB_r<32>(h, job, kind) : launch_rowTB_r<16>(h, job, kind);
    case AX_TWO:
        job.tw = o.tw; job.tw2 = o.tw2; job.pl = o.ptab;
        return paired_dispatch(job, [&](auto in_p, auto out_p) { return launch_rowT2_io<decltype(in_p)::value, decltype(out_p)::value>(h, job, kind); });
    case AX_FOURSTEP:
        job.tw = (&o == &h->opx) ? h->tw4_x : h->tw4_y;
        return o.R == 32 ? launch_rowT_r<32>(h, job, kind) : launch_rowT_r<16>(h, job, kind);
    default:
        return fail(h, MSL_ERR_STATE, "transposing pass: the axis has no one-pass kernel");
    }
}

// Slice loop when a grid length is 2 R^2: every pass transposes (there is no in-place kernel for those lengths).
// Pass k runs along y for even k and along x for odd k; after an odd number of slices one transpose brings the
// waves back to layout A, and the exit FFT is the stand-alone two-pass one.
int slice_loop_onepass_b(msl_handle* h, int fused_slot, int groups, int first_group) {
    const msl_config& c = h->cfg;
    const int P = c.n_probes * groups, nz = c.nz;           // images of this run: frames of the batch x probes
    const size_t toff = (size_t)first_group * c.nz * c.nx * c.ny;
    const size_t npix = (size_t)c.nx * c.ny;
    const long long isA = (long long)c.nx * h->pitch, isB = (long long)c.ny * h->pitchT;
    const bool fused = fused_slot >= 0;
    int rc;
    if ((rc = begin_timed(h, nz + 4 + (fused ? tap_launches(h) : 0)))) return rc;
    for (int k = 0; k < nz; ++k) {
        RowTJob j{};
        j.flags = (k > 0 ? P2_PRE_A : 0) | (k < nz - 1 ? P2_POST_A : 0);
        if (h->debug_flags_mask >= 0) j.flags &= h->debug_flags_mask;
        j.n_images = P;
        set_frame_groups(h, j, groups);
        if (h->opx.kind == AX_WAVE2K && h->opy.kind == AX_WAVE2K)     // work buffers between two of these passes: paired-lines layout
            j.flags |= (k > 0 ? P2_IN_PAIRED : 0) | (k < nz - 1 ? P2_OUT_PAIRED : 0);
        // 512-point lines next to 512 / 256 / 1024-point ones: interleaved line order between two passes (16-byte loads)
        if (interleaves(h->opx) && interleaves(h->opy) && !dbg_env("MSL_NO_INTERLEAVE") && h->debug_flags_mask < 0) {
            j.flags |= (k > 0 ? P2_IN_PAIRED : 0) | (k < nz - 1 ? P2_OUT_PAIRED : 0);
            j.perm_shift = (((k & 1) ? h->opy : h->opx).R == 32) ? 2 : 1;       // radix of the kernel that reads this pass's output
        }
        if (!(k & 1)) {
            j.in = (k == 0) ? h->psi0 : h->psi; j.out = h->psiT;
            j.trans = h->trans + toff + (size_t)k * npix; j.pl = h->pyt;
            j.in_image_stride = isA; j.out_image_stride = isB; j.in_pitch = h->pitch; j.out_pitch = h->pitchT; j.n_lines = c.nx;
            rc = launch_rowT_dir(h, h->opy, j, K_ROW);
        } else {
            j.in = h->psiT; j.out = h->psi;
            j.trans = h->transT + toff + (size_t)k * npix; j.pl = h->pxt;
            j.in_image_stride = isB; j.out_image_stride = isA; j.in_pitch = h->pitchT; j.out_pitch = h->pitch; j.n_lines = c.ny;
            rc = launch_rowT_dir(h, h->opx, j, K_COL);
        }
        if (rc) return rc;
        if (k < nz - 1) {
            int rp = 0;
            const int order = tap_order((k & 1) ? h->opx : h->opy, j.flags, j.perm_shift, &rp);
            if ((rc = tap_step(h, k, fused_slot, groups, (k & 1) ? h->psi : h->psiT, !(k & 1), order, rp, (k & 1) ? 1 : 0))) return rc;
        }
    }
    if (nz & 1) {
        dim3 grid((c.nx + 31) / 32, (c.ny + 31) / 32, P);
        hipLaunchKernelGGL(transpose_kernel, grid, dim3(256), 0, h->stream, h->psiT, h->psi, c.ny, c.nx, h->pitchT, h->pitch, isB, isA);
        HIPCHK(h, hipGetLastError());
        if ((rc = mark_launch(h, K_OTHER))) return rc;
    }
    if (fused) {
        if (h->Ry) {
            RowJob r = row_job(h, h->psi, P, h->pitch);
            r.do_fft = true;
            if ((rc = launch_row_fast(h, r, K_OTHER))) return rc;
        } else {
            LineArgs r = row_args(h, h->psi, h->psi, P, h->pitch);
            r.fft1 = +1;
            if ((rc = launch_lines(h, h->plan_y, r, K_OTHER))) return rc;
        }
        if ((rc = epilogue_x_pass(h, fused_slot, groups))) return rc;
    }
    count_slice_loop(h, P, groups, fused, 16);
    return MSL_OK;
}

template <int R>
int launch_row2_r(msl_handle* h, Row2Job job, int kind) {
    constexpr int N = R * R, G = 256 / R;
    const size_t lds = (size_t)N * 16 + (size_t)G * R * (R + 1) * 4;
    const int per_cu = std::max(1, std::min(2, (int)((size_t)h->lds_limit / lds)));
    const int grid = chunked_grid(h, job, job.nx / G, (long long)h->n_cus * per_cu);
    hipLaunchKernelGGL(row_pass2_kernel<R>, dim3(grid), dim3(256), lds, h->stream, job);
    HIPCHK(h, hipGetLastError());
    return mark_launch(h, kind);
}

// Slice loop with one HBM pass per slice (see fft_pow2.h).  Pass k runs along y when its distance to the last
// slice is even, else along x; all passes but the last write transposed, the last one is in place on layout A.
int slice_loop_onepass(msl_handle* h, int fused_slot, int groups, int first_group) {
    if (h->scheme_b) return slice_loop_onepass_b(h, fused_slot, groups, first_group);
    const msl_config& c = h->cfg;
    const int P = c.n_probes * groups, nz = c.nz;
    const size_t toff = (size_t)first_group * c.nz * c.nx * c.ny;
    const size_t npix = (size_t)c.nx * c.ny;
    const long long isA = (long long)c.nx * h->pitch, isB = (long long)c.ny * h->pitchT;
    const bool fused = fused_slot >= 0;
    int rc;
    if (nz == 1)
        HIPCHK(h, hipMemcpyAsync(h->psi, h->psi0, (size_t)P * isA * sizeof(float2), hipMemcpyDeviceToDevice, h->stream));
    if ((rc = begin_timed(h, nz + 2 + (fused ? tap_launches(h) : 0)))) return rc;
    for (int k = 0; k < nz; ++k) {
        const bool last = (k == nz - 1);
        int flags = (k > 0 ? P2_PRE_A : 0) | (!last ? P2_POST_A : 0) | ((last && fused) ? P2_POST_F : 0);
        if (h->debug_flags_mask >= 0) flags &= h->debug_flags_mask;     // timing experiments only (MSL_DEBUG_FLAGS_MASK)
        if (last) {
            Row2Job j{};
            j.psi = h->psi; j.trans = h->trans + toff + (size_t)k * npix; j.py = h->pyt; j.tw = h->tw4_y;
            j.image_stride = isA; j.pitch = h->pitch; j.nx = c.nx; j.n_images = P; j.flags = flags;
            set_frame_groups(h, j, groups);
            rc = h->Ry == 32 ? launch_row2_r<32>(h, j, K_ROW) : launch_row2_r<16>(h, j, K_ROW);
            if (rc) return rc;
            break;
        }
        const bool along_y = !slice_is_transposed(h, k);
        RowTJob j{};
        // between two transposing passes the work buffer is in the interleaved line order (16-byte loads in the reader): the first
        // pass reads the probes, the last transposing pass (k = nz - 2) writes for the in-place pass, both in natural order
        if (!dbg_env("MSL_NO_INTERLEAVE") && h->debug_flags_mask < 0) flags |= (k > 0 ? P2_IN_PAIRED : 0) | (k < nz - 2 ? P2_OUT_PAIRED : 0);
        j.flags = flags; j.n_images = P;
        j.perm_shift = ((along_y ? h->Rx : h->Ry) == 32) ? 2 : 1;             // radix of the kernel that reads this pass's output: log2(R' / 8)
        set_frame_groups(h, j, groups);
        if (along_y) {
            j.in = (k == 0) ? h->psi0 : h->psi; j.out = h->psiT;
            j.trans = h->trans + toff + (size_t)k * npix; j.pl = h->pyt; j.tw = h->tw4_y;
            j.in_image_stride = isA; j.out_image_stride = isB; j.in_pitch = h->pitch; j.out_pitch = h->pitchT; j.n_lines = c.nx;
            rc = h->Ry == 32 ? launch_rowT_r<32>(h, j, K_ROW) : launch_rowT_r<16>(h, j, K_ROW);
        } else {
            j.in = (k == 0) ? h->psi0T : h->psiT; j.out = h->psi;
            j.trans = h->transT + toff + (size_t)k * npix; j.pl = h->pxt; j.tw = h->tw4_x;
            j.in_image_stride = isB; j.out_image_stride = isA; j.in_pitch = h->pitchT; j.out_pitch = h->pitch; j.n_lines = c.ny;
            rc = h->Rx == 32 ? launch_rowT_r<32>(h, j, K_COL) : launch_rowT_r<16>(h, j, K_COL);
        }
        if (rc) return rc;
        const int order = (j.flags & P2_OUT_PAIRED) ? TAP_INTERLEAVED : TAP_NATURAL;
        if ((rc = tap_step(h, k, fused_slot, groups, along_y ? h->psiT : h->psi, along_y, order, 8 << j.perm_shift, along_y ? 0 : 1))) return rc;
    }
    if (fused && (rc = epilogue_x_pass(h, fused_slot, groups))) return rc;
    count_slice_loop(h, P, groups, fused, 16);
    return MSL_OK;
}

// n atoms of a frame group; `rows` rows of the sorted phase tables (the atoms plus the padding of every bin to SF_ALIGN rows)
int ensure_atoms(msl_handle* h, size_t n, size_t rows) {
    int rc;
    if (rows <= h->atom_cap) return (h->fin_R > 0 && h->d_wgt.n < h->atom_cap) ? h->d_wgt.alloc(h, h->atom_cap) : MSL_OK;
    (void)n;
    size_t cap = std::max<size_t>(rows, h->atom_cap * 3 / 2 + 1024);
    if (h->fin_R > 0 && (rc = h->d_wgt.alloc(h, cap))) return rc;         // (the weight of every row of a finite-projection build)
    if ((rc = h->d_pos.alloc(h, cap * 3)) || (rc = h->d_Z.alloc(h, cap)) || (rc = h->d_key.alloc(h, cap)) || (rc = h->d_order.alloc(h, cap)) ||
        (rc = h->d_u1.alloc(h, cap)) || (rc = h->d_u2.alloc(h, cap))) return rc;
    // phase tables: the quadrant kernel reads the columns 0 .. n/2 only
    if ((rc = h->d_ex.alloc(h, cap * (size_t)(h->cfg.nx / 2 + 1))) || (rc = h->d_ey.alloc(h, cap * (size_t)(h->cfg.ny / 2 + 1)))) return rc;
    h->atom_cap = cap;
    return MSL_OK;
}

// ---- per-slice sums: the TDS detector signal and the element maps (4.27); slice_sums.h ----
// A signal as the host sees it: the kernel policy plus its name in messages, the template slots N of a count n with their dispatch,
// the slots a (tile, image) of its slab is reserved with, and where the handle keeps its settings, weights and slab.
struct TdsSignal : TdsSums {
    static constexpr const char* name = "tds";
    static constexpr const char* setter = "msl_set_tds";
    static int slots(int n) { return n; }
    static int slab_slots(int n) { return n; }
    template <typename F> static void with_slots(int k, F&& f) { with_int<1, 2, 3, 4>(k, f); }
    static bool on(const msl_handle* h) { return h->tds_on; }
    static bool built(const msl_handle* h) { return h->tds_W && h->abs_built; }
    static int n(const msl_handle* h) { return h->tds_n; }
    static const float* weights(const msl_handle* h) { return h->tds_W; }
    static DevBuf<double>& slab(msl_handle* h) { return h->tds_part; }
};
struct IonSignal : IonSums {
    static constexpr const char* name = "ionization";
    static constexpr const char* setter = "msl_set_ionization";
    static int slots(int n) { return n <= 1 ? 1 : n <= 2 ? 2 : n <= 4 ? 4 : 8; }       // the next power of two
    static int slab_slots(int) { return ION_MAX; }          // (for any n: the slab is not reallocated between two launches of a loop)
    template <typename F> static void with_slots(int k, F&& f) { with_int<1, 2, 4, 8>(k, f); }
    static bool on(const msl_handle* h) { return h->ion_on; }
    static bool built(const msl_handle* h) { return h->ion_W && h->ion_built; }
    static int n(const msl_handle* h) { return h->ion_n; }
    static const float* weights(const msl_handle* h) { return h->ion_W; }
    static DevBuf<float>& slab(msl_handle* h) { return h->ion_part; }
};

// The reduction of P images at `psi` (the work buffers' layout) against n images of weights at w, w_cs values apart, into dst (P, n)
// float64, queued: the tile kernel into the signal's slab of partials, then the sums over the tiles in float64.  reps > 1 repeats the
// tile kernel (the timing of msl_tds_reduce / msl_ionization_reduce).
template <class S>
int slice_sums_queue(msl_handle* h, const float2* psi, int P, const float* w, size_t w_cs, int n, double* dst, int reps = 1) {
    const msl_config& c = h->cfg;
    const long long pairs = (long long)c.nx * ((c.ny + 1) / 2), n_tiles = (pairs + S::TILE - 1) / S::TILE;
    if (n_tiles > 0x7fffffffLL) return fail(h, MSL_ERR_UNSUPPORTED, "%s: too many tiles", S::name);
    const int slots = S::slots(n);
    auto& part = S::slab(h);
    int rc = part.reserve(h, (size_t)n_tiles * P * S::slab_slots(n));
    if (rc) return rc;
    // images per workgroup: as many as possible (the weights are loaded once per workgroup) while every slot still has a workgroup
    const long long wg_slots = (long long)h->n_cus * 8;
    int pc = P;
    while (pc > 1 && n_tiles * ((P + pc - 1) / pc) < wg_slots) pc = (pc + 1) / 2;
    while ((P + pc - 1) / pc > 65535) ++pc;
    const bool vec = (h->pitch % 2 == 0) && (((uintptr_t)psi & 15) == 0);
    const dim3 grid((unsigned)n_tiles, (unsigned)((P + pc - 1) / pc));
    for (int r = 0; r < reps; ++r) {
        S::with_slots(slots, [&](auto k) { with_bool(vec, [&](auto v) {
            hipLaunchKernelGGL((slice_sums_kernel<typename S::kernel_policy, decltype(k)::value, decltype(v)::value>), grid, dim3(256), 0, h->stream,
                               psi, w, (long long)w_cs, n, c.nx, c.ny, h->pitch, P, pc, part.p);
        }); });
        HIPCHK(h, hipGetLastError());
        if (reps == 1 && (rc = mark_launch(h, K_OTHER))) return rc;
    }
    S::with_slots(slots, [&](auto k) {
        hipLaunchKernelGGL((slice_sums_finish_kernel<typename S::acc_t, decltype(k)::value>), dim3((unsigned)(((long long)P * slots + 255) / 256)),
                           dim3(256), 0, h->stream, part.p, n_tiles, P, n, dst);
    });
    HIPCHK(h, hipGetLastError());
    return reps == 1 ? mark_launch(h, K_OTHER) : MSL_OK;
}

// The sums of signal S for P images at `psi` against the weights of slice z, into dst (P, n)
template <class S>
int slice_sums_of_slice(msl_handle* h, const float2* psi, int P, int z, double* dst, int reps = 1) {
    const size_t npix = (size_t)h->cfg.nx * h->cfg.ny;
    return slice_sums_queue<S>(h, psi, P, S::weights(h) + (size_t)z * npix, npix * h->cfg.nz, S::n(h), dst, reps);
}
// The store of msl_adjoint_add, queued where the reduction of a signal is: psi_z into slab z - 1 of the stack (psi_0 is psi0, which the
// loop leaves alone)
int adjoint_store_hook(msl_handle* h, int P, int z) {
    if (z == 0) return MSL_OK;
    const size_t slab = (size_t)P * h->cfg.nx * h->pitch;
    HIPCHK(h, hipMemcpyAsync(h->adj_stack + (size_t)(z - 1) * slab, h->psi, slab * sizeof(float2), hipMemcpyDeviceToDevice, h->stream));
    return mark_launch(h, K_OTHER);
}
// What the two-pass loop queues between the two launches of a slice's row step, where psi holds the wave arriving at slice z in real
// space: the sums of the active signal, into row z of its (nz, P, n) sums
int slice_sums_hook(msl_handle* h, int P, int z) {
    if (h->adj_on) return adjoint_store_hook(h, P, z);     // (msl_adjoint_add's loop: no signal is set next to the adjoint)
    return h->tds_on ? slice_sums_of_slice<TdsSignal>(h, h->psi, P, z, h->tds_acc + (size_t)z * P * h->tds_n)
                     : slice_sums_of_slice<IonSignal>(h, h->psi, P, z, h->ion_acc + (size_t)z * P * h->ion_n);
}

// out (nz, B, n) <- the sums (nz, n_probes, n) of the last slice loop, for the first B probes (B <= 0: all; *B is the count taken),
// queued on the stream: the caller waits for it
int slice_sums_fetch(msl_handle* h, const char* who, const double* sums, int n, int32_t* B, double* out) {
    const int P = h->cfg.n_probes;
    if (*B <= 0) *B = P;
    if (*B > P) return fail(h, MSL_ERR_INVALID, "%s: %d probes, the handle has %d", who, *B, P);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipMemcpy2DAsync(out, (size_t)*B * n * sizeof(double), sums, (size_t)P * n * sizeof(double), (size_t)*B * n * sizeof(double),
                               (size_t)h->cfg.nz, hipMemcpyDeviceToHost, h->stream));
    return MSL_OK;
}

// The reduction alone: the work buffer against the weights of one slice, `reps` times between two events
template <class S>
int slice_sums_reduce(msl_handle* h, const char* who, int32_t slice, int32_t reps, double* out, double* ms_reduce) {
    if (!h) return fail(h, MSL_ERR_INVALID, "%s: null handle", who);
    if (!S::on(h) || !S::built(h)) return fail(h, MSL_ERR_STATE, "%s: no weight stack (%s, then a build)", who, S::setter);
    if (slice < 0 || slice >= h->cfg.nz) return fail(h, MSL_ERR_INVALID, "%s: slice %d outside [0, %d)", who, slice, h->cfg.nz);
    if (reps < 1) return fail(h, MSL_ERR_INVALID, "%s: reps must be positive", who);
    const float2* src = h->psi.p;                       // MSL_BUF_EXIT: whatever the last slice loop left there
    const int P = h->cfg.n_probes, n = S::n(h);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    DevBuf<double> dst;
    int rc = dst.alloc(h, (size_t)P * n);
    if (rc) return rc;
    h->cur = nullptr;
    // the timed launches run between two events of their own, after one untimed pass has sized the slab
    if (reps > 1 && (rc = slice_sums_of_slice<S>(h, src, P, slice, dst))) return rc;
    double ms = 0.0;
    EventPair timer;
    if ((rc = timer.begin(h)) || (rc = slice_sums_of_slice<S>(h, src, P, slice, dst, reps)) || (rc = timer.end(h, &ms))) {
        (void)hipStreamSynchronize(h->stream);          // nothing queued reads dst when it is freed
        return rc;
    }
    if (ms_reduce) *ms_reduce = ms / reps;              // (the one finishing sum of the call is in it: take reps large)
    if (out) HIPCHK(h, hipMemcpy(out, dst, (size_t)P * n * sizeof(double), hipMemcpyDeviceToHost));
    return MSL_OK;
}

// The slice loop (generic kernels).  fused_slot < 0: leave real-space exit waves in psi.
// While a per-slice signal is on (msl_set_tds or msl_set_ionization) the row step of every slice is issued as two launches of its own
// kernels -- the inverse y-transform alone, as fft2_inplace issues it, then t_s, the forward transform and P_y -- so that between them
// psi holds psi_s in real space at its true scale, where the reduction is queued (at s = 0 psi is psi0).  Every elastic launch computes
// what the single launch computes; the per-slice sums go to tds_acc (nz, P, tds_n) or ion_acc (nz, P, ion_n), and for the ionisation
// signal the norms of the incident waves, the same kernel against an image of ones, to ion_norm.  `signal` is run_loop's alone: every
// other caller (msl_smatrix_build) runs the plain loop and leaves the sums of the last probe loop alone, whatever the handle's setting.
// `store` is msl_adjoint_add's alone: the same split row step, where the hook then copies psi into the wave stack (never with `signal`).
int slice_loop(msl_handle* h, int fused_slot, int groups, int first_group, bool signal = false, bool store = false) {
    const msl_config& c = h->cfg;
    const bool tds = signal && h->tds_on, ion = signal && !tds;
    const bool sums = signal || store;                      // the split row step with the hook between its halves
    h->pm_g = 0;                                            // the work buffer is rewritten
    if (store && (signal || !h->adj_on || groups != 1 || h->onepass))
        return fail(h, MSL_ERR_STATE, "adjoint: the slice loop needs one frame per launch on the two-pass loop");
    if (signal && (groups != 1 || h->onepass))
        return fail(h, MSL_ERR_STATE, "%s: the slice loop needs one frame per launch on the two-pass loop", ion ? "ionization" : "tds");
    if (tds && !TdsSignal::built(h)) return fail(h, MSL_ERR_STATE, "tds: no weight stack (build the potential after msl_set_tds)");
    if (ion && !IonSignal::built(h))
        return fail(h, MSL_ERR_STATE, "ionization: no weight stack (build the potential after msl_set_ionization)");
    if (h->onepass) return slice_loop_onepass(h, fused_slot, groups, first_group);
    const int P = c.n_probes * groups, nz = c.nz;
    const size_t npix = (size_t)c.nx * c.ny;
    const size_t toff = (size_t)first_group * c.nz * npix;
    int rc;
    if (signal && (rc = (ion ? h->ion_acc : h->tds_acc).reserve(h, (size_t)nz * P * (ion ? h->ion_n : h->tds_n)))) return rc;
    if (ion && (rc = h->ion_norm.reserve(h, (size_t)P))) return rc;
    HIPCHK(h, hipMemcpyAsync(h->psi, h->psi0, (size_t)P * c.nx * h->pitch * sizeof(float2), hipMemcpyDeviceToDevice, h->stream));
    if (ion && (rc = slice_sums_queue<IonSignal>(h, h->psi, P, h->ion_ones, npix, 1, h->ion_norm))) return rc;     // (ahead of the timed launches)
    const bool fused = fused_slot >= 0;
    if ((rc = begin_timed(h, (sums ? 5 : 2) * nz + 2 + (fused ? tap_launches(h) : 0)))) return rc;
    // the row step of slice z, or one of its halves: the inverse y-transform of the previous step; t_z, the forward transform and P_y
    auto row_step = [&](int z, bool inverse, bool forward) {
        const bool last = (z == nz - 1);
        if (h->Ry) {
            RowJob r = row_job(h, h->psi, P, h->pitch);
            r.do_ifft = inverse;
            if (forward) { r.trans = h->trans + toff + (size_t)z * npix; r.do_fft = (!last || fused); r.py = last ? nullptr : h->pyt; }
            set_frame_groups(h, r, groups);
            return launch_row_fast(h, r, K_ROW);
        }
        LineArgs r = row_args(h, h->psi, h->psi, P, h->pitch);
        r.fft1 = inverse ? -1 : 0;
        if (groups > 1) { r.group = c.n_probes; r.m_gs = (long long)c.nz * npix; r.out_gs = (long long)c.n_probes * r.out_is; }
        if (forward) {
            r.m1_kind = MUL_ARRAY; r.m1 = h->trans + toff + (size_t)z * npix; r.m1_ls = c.ny;
            if (!last) { r.fft2 = +1; r.m2_kind = MUL_VEC; r.m2 = h->pyt; }
            else if (fused) { r.fft2 = +1; }
        }
        return launch_lines(h, h->plan_y, r, K_ROW);
    };
    for (int z = 0; z < nz; ++z) {
        const bool last = (z == nz - 1);
        if (sums) {
            if ((z > 0 && (rc = row_step(z, true, false))) || (rc = slice_sums_hook(h, P, z)) || (rc = row_step(z, false, true))) return rc;
        } else if ((rc = row_step(z, z > 0, true))) {
            return rc;
        }
        if (!last && (rc = tap_step(h, z, fused_slot, groups, h->psi, false, TAP_NATURAL, 8, 2))) return rc;
        if (!last) {
            if (h->Rx) {
                ColJob k = col_job(h, h->psi, h->psi, P, h->pitch, h->pitch);
                k.px = h->pxt; k.flags = COL_FWD | COL_MULPX | COL_INV;
                if ((rc = launch_col_fast(h, k, K_COL))) return rc;
            } else {
                LineArgs k = col_args(h, h->psi, h->psi, P, h->pitch, h->pitch);
                k.fft1 = +1; k.m1_kind = MUL_VEC; k.m1 = h->pxt; k.fft2 = -1;
                if ((rc = launch_lines(h, h->plan_x, k, K_COL))) return rc;
            }
        }
    }
    if (fused) {
        // epilogue: fft along x, fftshift both axes, scatter into (P, T_local, nx, ny)
        if ((rc = epilogue_x_pass(h, fused_slot, groups))) return rc;
    }
    if (!signal) {
        count_slice_loop(h, P, groups, fused, store ? 32 + 16 + 16 : 32);      // (the split row step, and the copy into the stack)
        return MSL_OK;
    }
    (ion ? h->ion_have : h->tds_have) = true;
    // 16 B more per pixel and slice-step for the split row step, 8 for the reduction's read, and the weights once per image chunk
    count_slice_loop(h, P, groups, fused, 32 + 16 + 8);
    if (!ion) h->ctr.algorithmic_bytes += (uint64_t)nz * h->tds_n * 4ull * npix;
    else h->ctr.algorithmic_bytes += (uint64_t)nz * h->ion_n * 4ull * npix + 8ull * P * npix;      // (and the norm's read of psi0)
    return MSL_OK;
}

// ---- gradients: the slice loop backwards; adjoint.h ----
// The step of slice s for the first B images of g (the work buffer's layout), queued: psi_s from the stack (psi0 at s = 0), t_s of the
// current batch slot, row s of the accumulator
// adjoint_step_kernel<VEC> or not: an even pitch and g, psi0 and the stack on 16 bytes
bool adjoint_step_vec(const msl_handle* h, const float2* g) {
    return (h->pitch % 2 == 0) && (((uintptr_t)g & 15) == 0) && (((uintptr_t)h->psi0.p & 15) == 0) && (((uintptr_t)h->adj_stack.p & 15) == 0);
}
int adjoint_step_launch(msl_handle* h, float2* g, int s, int B) {
    const msl_config& c = h->cfg;
    const size_t npix = (size_t)c.nx * c.ny, slab = (size_t)c.n_probes * c.nx * h->pitch;
    const long long pairs = (long long)c.nx * ((c.ny + 1) / 2), step_tiles = (pairs + ADJ_TILE - 1) / ADJ_TILE;
    const bool vec = adjoint_step_vec(h, g);
    const float2* psi_s = s == 0 ? h->psi0.p : h->adj_stack.p + (size_t)(s - 1) * slab;
    const float2* t = h->trans + ((size_t)h->cur_batch * c.nz + s) * npix;
    double* grad = h->adj_grad + (size_t)s * npix;
    if (vec) hipLaunchKernelGGL(adjoint_step_kernel<true>, dim3((unsigned)step_tiles), dim3(256), 0, h->stream, g, psi_s, t, c.nx, c.ny, h->pitch, B, 2.0 * c.sigma, grad);
    else hipLaunchKernelGGL(adjoint_step_kernel<false>, dim3((unsigned)step_tiles), dim3(256), 0, h->stream, g, psi_s, t, c.nx, c.ny, h->pitch, B, 2.0 * c.sigma, grad);
    HIPCHK(h, hipGetLastError());
    return MSL_OK;
}

// One probe batch: the forward loop with the store, the exit FFT, the residual pass against the data D (B, nx, ny) on the host, and the
// backward loop, which adds the batch's share into the accumulator.  loss_out (B) float64; probe_grad (B, nx, ny) c64 or null.  Waits
// for the stream.
int adjoint_add(msl_handle* h, const float* data, int B, double* loss_out, float2* probe_grad) {
    const msl_config& c = h->cfg;
    const int P = c.n_probes, nz = c.nz;
    const size_t npix = (size_t)c.nx * c.ny;
    const long long res_tiles = ((long long)npix + ADJ_RES_TILE - 1) / ADJ_RES_TILE;
    const long long pairs = (long long)c.nx * ((c.ny + 1) / 2), step_tiles = (pairs + ADJ_TILE - 1) / ADJ_TILE;
    if (res_tiles > 0x7fffffffLL || step_tiles > 0x7fffffffLL || B > 65535) return fail(h, MSL_ERR_UNSUPPORTED, "msl_adjoint_add: too many tiles");
    int rc;
    if ((rc = h->adj_part.reserve(h, (size_t)res_tiles * P))) return rc;
    HIPCHK(h, hipMemcpyAsync(h->adj_D, data, (size_t)B * npix * sizeof(float), hipMemcpyHostToDevice, h->stream));
    if ((rc = slice_loop(h, -1, 1, h->cur_batch, false, true))) return rc;
    h->have_exit = false;                                   // psi ends as the probe gradient
    float2* g = h->psi;
    if ((rc = fft2_inplace(h, g, B, +1, 1.0f, h->pitch))) return rc;
    const dim3 res_grid((unsigned)res_tiles, (unsigned)B);
    const float* w = h->adj_w;
    switch (h->adj_on) {
        case ADJ_AMPLITUDE: hipLaunchKernelGGL(adjoint_residual_kernel<ADJ_AMPLITUDE>, res_grid, dim3(256), 0, h->stream, g, (const float*)h->adj_D, w, c.nx, c.ny, h->pitch, B, h->adj_eps, h->adj_part.p); break;
        case ADJ_INTENSITY: hipLaunchKernelGGL(adjoint_residual_kernel<ADJ_INTENSITY>, res_grid, dim3(256), 0, h->stream, g, (const float*)h->adj_D, w, c.nx, c.ny, h->pitch, B, h->adj_eps, h->adj_part.p); break;
        default: hipLaunchKernelGGL(adjoint_residual_kernel<ADJ_POISSON>, res_grid, dim3(256), 0, h->stream, g, (const float*)h->adj_D, w, c.nx, c.ny, h->pitch, B, h->adj_eps, h->adj_part.p); break;
    }
    hipLaunchKernelGGL((slice_sums_finish_kernel<double, 1>), dim3((unsigned)((B + 255) / 256)), dim3(256), 0, h->stream, (const double*)h->adj_part.p,
                       res_tiles, B, 1, h->adj_loss.p);
    HIPCHK(h, hipGetLastError());
    if ((rc = fft2_inplace(h, g, B, -1, 1.0f, h->pitch))) return rc;     // g = N ifft2(G): the adjoint of the unnormalised transform
    const long long total = (long long)B * c.nx * c.ny;
    for (int s = nz - 1; s >= 0; --s) {
        if ((rc = adjoint_step_launch(h, g, s, B))) return rc;
        if (s == 0) break;
        if ((rc = fft2_inplace(h, g, B, +1, 1.0f, h->pitch))) return rc;
        hipLaunchKernelGGL(adjoint_conjprop_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->stream, g, (const float2*)h->pxt.p,
                           (const float2*)h->pyt.p, c.nx, c.ny, h->pitch, total);
        HIPCHK(h, hipGetLastError());
        if ((rc = fft2_inplace(h, g, B, -1, 1.0f, h->pitch))) return rc;
    }
    // per image: the two exit transforms (64 B per pixel), the residual (16 + 4), per slice the step (24) and per propagation the
    // product and its two transforms (16 + 64); per call t_s and the accumulator (8 + 16 per pixel and slice)
    h->ctr.algorithmic_bytes += (uint64_t)B * npix * (84ull + 24ull * nz + 80ull * (nz - 1)) + 24ull * nz * npix;
    HIPCHK(h, hipMemcpyAsync(loss_out, h->adj_loss, (size_t)B * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (probe_grad)
        HIPCHK(h, hipMemcpy2DAsync(probe_grad, (size_t)c.ny * sizeof(float2), g, (size_t)h->pitch * sizeof(float2), (size_t)c.ny * sizeof(float2),
                                   (size_t)B * c.nx, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->pm_g = B;                                            // the probe gradient of B images: what msl_adjoint_probe_params(NULL) reads
    return MSL_OK;
}

// ---- gradients with respect to atom positions: the potential build backwards; adjoint.h ----
// The tiles of position_gradient_kernel from the bin starts of the resident build (a small download: the call is synchronous anyway):
// every (slice, species) bin in PG_ATOMS rows at a time, in bin order, so that the tiles of a slice are neighbours.  tile_of[s] = the
// first tile of slice s (tile_of[nz] = all of them); bins_used = bins that hold rows
int position_tiles(msl_handle* h, std::vector<int>& tile_of, int& bins_used, int& rows) {
    const int nz = h->cfg.nz, nsp = h->pg_nsp, nkeys = nz * nsp;
    tile_of.assign((size_t)nz + 1, 0);
    bins_used = rows = 0;
    if (h->pg_n == 0 || nsp == 0) return MSL_OK;         // (a build without atoms sorts nothing)
    std::vector<int> start((size_t)nkeys + 1);
    HIPCHK(h, hipMemcpyAsync(start.data(), h->d_start, start.size() * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    std::vector<int4> tiles;
    for (int s = 0; s < nz; ++s) {
        tile_of[s] = (int)tiles.size();
        for (int sp = 0; sp < nsp; ++sp) {
            const int a0 = start[(size_t)s * nsp + sp], a1 = start[(size_t)s * nsp + sp + 1];
            if (a1 > a0) ++bins_used;
            for (int a = a0; a < a1; a += PG_ATOMS) tiles.push_back(make_int4(s, sp, a, std::min(PG_ATOMS, a1 - a)));
        }
    }
    tile_of[nz] = (int)tiles.size();
    rows = start[nkeys];
    int rc;
    if ((rc = h->pg_tiles.reserve(h, tiles.size()))) return rc;
    if (!tiles.empty()) {
        HIPCHK(h, hipMemcpyAsync(h->pg_tiles, tiles.data(), tiles.size() * sizeof(int4), hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));        // (the list is a local of this call)
    }
    return MSL_OK;
}

// Gamma (nz, nx, ny) float64 on the device -> pg_out (pg_n, 3), queued: per chunk of slices the c64 images, fft2_inplace(+1) and the
// tiles of those slices
int position_chain(msl_handle* h, const double* d_gamma, const std::vector<int>& tile_of) {
    const msl_config& c = h->cfg;
    const size_t npix = (size_t)c.nx * c.ny;
    const int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)c.nz, ((size_t)256 << 20) / (npix * sizeof(float2))));
    int rc;
    if ((rc = h->pg_img.reserve(h, (size_t)chunk * npix))) return rc;
    HIPCHK(h, hipMemsetAsync(h->pg_out, 0, (size_t)std::max<int64_t>(1, h->pg_n) * 3 * sizeof(double), h->stream));
    const double cc = 2.0 * M_PI / ((double)npix * c.dx * c.dx * c.dy * c.dy);
    for (int s0 = 0; s0 < c.nz; s0 += chunk) {
        const int ns = std::min(chunk, c.nz - s0), t0 = tile_of[s0], t1 = tile_of[s0 + ns];
        if (t1 == t0) continue;
        const long long total = (long long)ns * (long long)npix;
        hipLaunchKernelGGL(position_gamma_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->stream, d_gamma + (size_t)s0 * npix,
                           h->pg_img.p, total);
        HIPCHK(h, hipGetLastError());
        if ((rc = fft2_inplace(h, h->pg_img, ns, +1, 1.0f, c.ny))) return rc;
        hipLaunchKernelGGL(position_gradient_kernel, dim3((unsigned)(t1 - t0)), dim3(256), 0, h->stream, (const int4*)h->pg_tiles.p + t0,
                           (const float2*)h->pg_img.p, s0, (const float2*)h->d_ex.p, (const float2*)h->d_ey.p, (const float*)h->d_ff.p,
                           (const int*)h->d_order.p, c.nx, c.ny, c.nx / 2 + 1, c.ny / 2 + 1, (float)(1.0 / (c.nx * c.dx)), (float)(1.0 / (c.ny * c.dy)),
                           cc, h->pg_ax1, h->pg_ax2, h->pg_out.p);
        HIPCHK(h, hipGetLastError());
        if ((rc = mark_launch(h, K_OTHER))) return rc;
    }
    return MSL_OK;
}

// the state both entry points need; d_gamma: the accumulator, or the caller's Gamma uploaded
int position_prepare(msl_handle* h, const char* who, const double* gamma, const double** d_gamma) {
    if (!h->pg_valid || !h->have_potential)
        return fail(h, MSL_ERR_STATE, "%s: no single-frame msl_build_potential is resident (its phase tables, order and bins are what the "
                                      "chain reads: a later build of several frames, msl_build_thermal / msl_build_modes, msl_upload_potential, "
                                      "msl_set_projection or msl_set_absorption dropped them)", who);
    if (!gamma && !h->adj_on) return fail(h, MSL_ERR_STATE, "%s: gamma == NULL needs the accumulator of msl_set_adjoint", who);
    const msl_config& c = h->cfg;
    const size_t npix = (size_t)c.nx * c.ny;
    int rc;
    if ((rc = h->pg_out.reserve(h, (size_t)std::max<int64_t>(1, h->pg_n) * 3))) return rc;
    if (gamma) {
        if ((rc = h->pg_gamma.reserve(h, (size_t)c.nz * npix))) return rc;
        HIPCHK(h, hipMemcpyAsync(h->pg_gamma, gamma, (size_t)c.nz * npix * sizeof(double), hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));        // (the caller's memory is pageable)
    }
    *d_gamma = gamma ? h->pg_gamma.p : h->adj_grad.p;
    return MSL_OK;
}

// cyclic length of the convolution that IS the propagation along an axis of a convolution kind (0: none), and the entries of its filter qf
int conv_len(const msl_handle::OpDir& o) { return o.base == AX_CONV ? o.R * o.R : o.base == AX_CONV2K ? 2048 : o.base == AX_CONV4K ? 4096 : 0; }
size_t conv_filter_entries(const msl_handle::OpDir& o) { return o.base == AX_CONV4K ? 2052 : (size_t)conv_len(o) / 2 + 2; }

// ---- axis planning ----------------------------------------------------------------------------------
// The kind of the slice loop's pass along an axis of n points (n_other lines per image; Rfast = the four-step radix of the axis or 0;
// plan_M = the length of its generic plan, > n for a Bluestein plan).  want = false (two-pass loop asked for): no one-pass kind.
void plan_axis_kind(const msl_handle* h, msl_handle::OpDir& o, int n, int n_other, int Rfast, int plan_M, bool want) {
    const bool lines_ok = (n_other % 16 == 0);          // the register kernels take 16 lines at a time
    AxisKind base = AX_NONE;
    if (!want) {
    } else if (Rfast && lines_ok) {
        base = AX_FOURSTEP;
    } else if ((n == 512 || n == 2048) && lines_ok && !dbg_env("MSL_NO_TWO")) {
        // 512 = 2 R^2 points on the R = 16 register kernels; 2048-point lines on the wave-per-line FFT
        base = n == 512 ? AX_TWO : AX_WAVE2K;
    } else if (n >= 33 && n <= 512 && (n <= 128 || n >= 192 || plan_M != n) && !dbg_env("MSL_NO_BLUESTEIN_REG")) {
        // zero-padded cyclic convolution (or, MSL_CHIRPZ=1, chirp-z) on the register FFTs of length M = R^2 >= 2n - 1.  A line
        // costs the same whatever n is, so against the generic Stockham kernel (cost ~ n log n) it wins for n <= 128 (M = 256)
        // and from n ~ 190 up (M = 1024; 64 probes x 50 slices: 160^2 1.83 M vs 1.72 M slice-steps/s, 200^2 1.23 vs 1.31 M,
        // 240^2 0.84 vs 1.13 M), and everywhere the generic kernel would need its own LDS-resident Bluestein transform
        base = AX_CONV;
    } else if (n >= 513 && n <= 1024 && !dbg_env("MSL_NO_BLUESTEIN_REG")) {
        // 513..1024: the same on the wave-per-line 2048-point register FFT, every length (convolution form against the
        // Stockham kernel: 540^2 102 k -> 186 k slice-steps/s, 600^2 85 k -> 160 k, 768^2 73 k -> 130 k)
        base = AX_CONV2K;
    } else if (n >= 1025 && n <= 2047 && !dbg_env("MSL_NO_CONV4096") && !dbg_env("MSL_NO_BLUESTEIN_REG")) {
        // 1025..2047: cyclic convolution of length 4096 on pairs of 2048-point wave FFTs, the two branches of the radix-2
        // step on two waves (rowTC2_pass_kernel): 16 probes x 20 slices, slice-steps/s against the generic two-pass loop:
        // 1100^2 19.6 k -> 27.5 k, 1500^2 12.6 k -> 18.3 k, 2000^2 6.8 k -> 11.4 k.  MSL_CONV4096=1 selects the first
        // version, both branches in one wave (rowTC_pass_kernel): two 64-register line sets plus the transform's
        // temporaries spill 916 B per lane and it is no faster than the generic loop (20.0 k at 1100^2).
        base = AX_CONV4K;
    } else if (plan_M <= 1024 && !dbg_env("MSL_NO_GENERIC_ONEPASS")) {
        // generic LDS kernel with a transposing store: tiles of >= 8 lines keep the stores at 64 bytes or more
        base = AX_GENERIC;
    }
    // smooth lengths A * B (A, B <= 32) or 2 A * B (up to 1728) with a compiled kernel: direct mixed-radix passes in the slice
    // loop (600^2: 163 k -> 330 k slice-steps/s, 1500^2: 18 k -> 55 k), over the base kind the length gets otherwise
    int mA = 0, mB = 0, mG = 0;
    const bool mixed = want && base != AX_FOURSTEP && base != AX_TWO && base != AX_WAVE2K && rowTM_factors(n, &mA, &mB, &mG) &&
                       !dbg_env("MSL_NO_MIXED") && (mG == 64 ? rowTM2_lds_bytes(mA, mB) : rowTM_lds_bytes(mA, mB)) <= (size_t)h->lds_limit;
    o.n = n;
    o.base = base;
    o.kind = mixed ? AX_MIXED : base;
    o.R = base == AX_FOURSTEP ? Rfast : base == AX_TWO ? 16 : base == AX_CONV ? (n <= 128 ? 16 : 32) :
          (base == AX_WAVE2K || base == AX_CONV2K || base == AX_CONV4K) ? 32 : 0;
}

// The tables of axis o (msl_handle::OpDir); `other` = the other axis, planned
int make_axis_tables(msl_handle* h, msl_handle::OpDir& o, const msl_handle::OpDir& other) {
    const int n = o.n;
    int rc = MSL_OK;
    if (o.kind == AX_MIXED) {
        int mA = 0, mB = 0, mG = 0;
        rowTM_factors(n, &mA, &mB, &mG);
        const int lanes1 = mG == 64 ? 2 * mA : mA;           // lanes of layout 1 (rowtm_pass.h)
        std::vector<float2> T(2 * (size_t)n + (mG == 64 ? 2 * mA : 0));
        for (int k2 = 0; k2 < mB; ++k2)
            for (int n1 = 0; n1 < lanes1; ++n1) {
                const double a = -2.0 * M_PI * (double)((k2 * n1) % n) / (double)n;
                const float2 w = make_float2((float)cos(a), (float)sin(a));
                T[k2 * lanes1 + n1] = w;
                if (mG == 64) T[n + (n1 % mA) * 2 * mB + 2 * k2 + n1 / mA] = w;      // lane order of layout 2: [m 2B + 2 k2 + h], n1 = m + A h
                else T[n + n1 * mB + k2] = w;
            }
        if (mG == 64)
            for (int m = 0; m < mA; ++m) {
                const double a = -2.0 * M_PI * (double)m / (double)(2 * mA);
                T[2 * n + m] = make_float2(1.f, 0.f);
                T[2 * n + mA + m] = make_float2((float)cos(a), (float)sin(a));
            }
        if ((rc = upload(h, o.mtw, T))) return rc;
    }
    switch (o.base) {
    case AX_TWO: {
        std::vector<float2> t(o.R * o.R);
        for (int m = 0; m < o.R * o.R; ++m) {
            const double a = -2.0 * M_PI * (double)m / (double)n;
            t[m] = make_float2((float)cos(a), (float)sin(a));
        }
        if ((rc = make_tw4(h, o.tw, o.R)) || (rc = upload(h, o.tw2, t)) || (rc = o.ptab.alloc(h, (size_t)n))) return rc;
        break;
    }
    case AX_WAVE2K:
        if ((rc = make_wave2k_tables(h, o.tw, o.tw2))) return rc;
        break;
    case AX_CONV:
    case AX_CONV2K:
        if ((rc = make_cz_tables(h, o.cz, n)) || (rc = o.qf.alloc(h, conv_filter_entries(o)))) return rc;
        break;
    case AX_CONV4K: {
        std::vector<float2> wq(2048);
        for (int i = 0; i < 2048; ++i) {
            const double a = -2.0 * M_PI * (double)i / 4096.0;
            wq[i] = make_float2((float)cos(a), (float)sin(a));
        }
        if ((rc = make_wave2k_tables(h, o.tw, o.tw2)) || (rc = upload(h, o.bw, wq)) || (rc = o.qf.alloc(h, conv_filter_entries(o)))) return rc;
        break;
    }
    default:
        break;
    }
    // an axis of at most 1024 points next to a convolution axis gets chirp-z tables too, so that the potential's inverse transform
    // runs on the register kernels along both (512 x 300, 349 x 1024 ...)
    auto conv = [](const msl_handle::OpDir& d) { return d.base == AX_CONV || d.base == AX_CONV2K; };
    if (!conv(o) && conv(other) && n >= 33 && n <= 1024) return make_cz_tables(h, o.cz, n);
    return MSL_OK;
}

// ---- potential build ----------------------------------------------------------
// The form of the potential's inverse transform for the planned axes.  A transposing form stores the slices a pass along x reads
// into transT itself, which a kept V rules out (V is written by the untransposed store only).
PotIfft plan_pot_ifft(const msl_handle* h) {
    if (!h->onepass || h->V) return PI_LINES;
    if (h->opx.base == AX_WAVE2K && h->opy.base == AX_WAVE2K && h->transT) return PI_WAVE2K;
    if (h->transT && h->opx.cz.R && h->opy.cz.R) return PI_CHIRPZ;                     // chirp-z tables along both axes
    if (h->opx.base == AX_TWO && h->opy.base == AX_TWO) return PI_TWO;
    return PI_LINES;
}

// R_s is Hermitian (real V): only the rows kx <= nx/2 are written and row-transformed when the inverse transform mirrors them itself
// (every register-kernel path: col_pass_kernel<.., HERM> with four-step kernels on both axes, ifftT2 / ifftTB / ifftTW with job.herm)
bool pot_half_rows(const msl_handle* h) { return h->pot_ifft != PI_LINES || (h->Rx && h->Ry); }

// what the stages of build_potentials share: the constants of the call and the group of g frames they work on
struct PotGroup {
    int z2s[104], species[104], nsp;    // species present, sorted ascending like np.unique: z2s[Z] = index into species, -1 where Z does not occur
    int64_t n; int32_t ax1, ax2, axs;   // atoms per frame; the axes the caller's positions are read along
    int keys_per_frame;             // (slice, species) bins per frame
    // finite projection: rep = 2 (2 R + 1) rows per atom and ntab = nsp (2 R + 1) J channel tables; without it rep = 1 and ntab = nsp.
    // The tables are the "species" of the sort and of the structure factor; z2s / species stay indexed by species
    int rep, ntab; bool finite;
    int cx, cy; float vscale;       // table columns the quadrant kernel reads: the frequencies 0 .. n/2
    bool half_rows, sf_stream;      // pot_half_rows; many atoms per bin: the streaming structure-factor kernel, whose bins are padded to whole half-trips
    int g, slot, n_slices, nkeys;   // frames, first batch slot, slices and bins of the group
    long long rows, rows_pad;       // rows (atoms x rep) of the group; sorted table rows at most: every bin padded to SF_ALIGN
    float2* TR; float2* TRT;        // batch slots this group's stacks go to (trans, transT)
};

// Forget the phonon modes and return their device memory (the stream is idle: the callers have synchronised)
void drop_modes(msl_handle* h) {
    h->have_modes = false;
    h->md_basis.release(); h->md_q.release(); h->md_tau.release(); h->md_W.release(); h->md_C.release();
    h->md_M = h->md_nb = 0;
}

int map_species(msl_handle* h, const int32_t* Z, int64_t n, PotGroup& m) {
    for (int i = 0; i < 104; ++i) m.z2s[i] = -1;
    for (int64_t a = 0; a < n; ++a) {
        if (Z[a] < 1 || Z[a] > 103) return fail(h, MSL_ERR_INVALID, "msl_build_potential: atomic number %d out of 1..103", Z[a]);
        m.z2s[Z[a]] = 0;
    }
    m.nsp = 0;
    for (int z = 1; z <= 103; ++z) if (m.z2s[z] == 0) { m.z2s[z] = m.nsp; m.species[m.nsp++] = z; }
    return MSL_OK;
}

// Per-frame inputs of a group, host -> device: the positions `pos` of its frames and, with the first group of a call, the species
// maps and Z.  They go through pinned staging (msl_handle::HostStage) so that no pointer into caller memory is kept.
int stage_atoms(msl_handle* h, const PotGroup& p, const double* pos, const int32_t* Z, bool send_maps) {
    msl_handle::HostStage& st = h->stage[h->stage_pos++ & 1];
    if (!st.ev) HIPCHK(h, hipEventCreateWithFlags(&st.ev, hipEventDisableTiming));
    if (st.used) HIPCHK(h, hipEventSynchronize(st.ev));            // the copies queued from this slot two calls ago
    const size_t z_bytes = (size_t)p.n * sizeof(int), pos_bytes = (size_t)p.n * p.g * 3 * sizeof(double);
    const size_t off_sp = sizeof p.z2s, off_Z = (off_sp + sizeof p.species + 7) & ~(size_t)7;
    const size_t off_pos = (off_Z + z_bytes + 7) & ~(size_t)7, need = off_pos + pos_bytes;
    if (need > st.bytes) {
        if (st.buf) (void)hipHostFree(st.buf);
        st.buf = nullptr; st.bytes = 0;
        const size_t cap = need + need / 4;
        if (hipHostMalloc((void**)&st.buf, cap, hipHostMallocDefault) != hipSuccess)
            return fail(h, MSL_ERR_NOMEM, "hipHostMalloc(%zu bytes) failed", cap);
        st.bytes = cap;
    }
    memcpy(st.buf + off_pos, pos, pos_bytes);
    if (send_maps) {
        memcpy(st.buf, p.z2s, sizeof p.z2s);
        memcpy(st.buf + off_sp, p.species, sizeof p.species);
        memcpy(st.buf + off_Z, Z, z_bytes);
        HIPCHK(h, hipMemcpyAsync(h->d_z2s, st.buf, sizeof p.z2s, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(h->d_species, st.buf + off_sp, p.nsp * sizeof(int), hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(h->d_Z, st.buf + off_Z, z_bytes, hipMemcpyHostToDevice, h->stream));
    }
    HIPCHK(h, hipMemcpyAsync(h->d_pos, st.buf + off_pos, pos_bytes, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipEventRecord(st.ev, h->stream));
    st.used = true;
    return MSL_OK;
}

// The generated source of build_potentials: frames first .. of the handle's resident structure, Einstein-model configurations
// (msl_build_thermal) or, with `modes`, frames synthesised from the resident phonon modes (msl_build_modes)
struct GeneratedSource { bool modes; uint64_t seed; uint64_t first; };

// What stage_atoms sends with the first group of a call, for a generated source: the resident species maps and Z, device to device
int stage_resident_maps(msl_handle* h, const PotGroup& p) {
    HIPCHK(h, hipMemcpyAsync(h->d_z2s, h->th_z2s, sizeof p.z2s, hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->d_species, h->th_species, p.nsp * sizeof(int), hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->d_Z, h->th_Z, (size_t)p.n * sizeof(int), hipMemcpyDeviceToDevice, h->stream));
    return MSL_OK;
}

// stage_atoms for a group of configurations: the positions are generated into d_pos on the device (thermal_positions_kernel, one
// thread per configuration and atom); with the first group of a call the resident species maps and Z are copied, device to device,
// to where stage_atoms puts them.  No pinned staging, no host copy.
int stage_thermal(msl_handle* h, const PotGroup& p, uint64_t seed, uint64_t first_config, bool send_maps) {
    int rc;
    if (send_maps && (rc = stage_resident_maps(h, p))) return rc;
    hipLaunchKernelGGL(thermal_positions_kernel, dim3((unsigned)(((long long)p.n * p.g + 255) / 256)), dim3(256), 0, h->stream, h->th_pos0, h->th_sigma,
                       (long long)p.n, p.g, (unsigned long long)seed, (unsigned long long)first_config, h->d_pos);
    HIPCHK(h, hipGetLastError());
    return MSL_OK;
}

// The frames first_frame .. first_frame + count - 1 of the resident modes into `pos` (count, n, 3): the coefficient table C
// (mode_coefficients_kernel, count x M threads), then one thread per atom and tile of 8 frames -- of 2 for a group of one or two
// frames -- (mode_positions_kernel).
// count <= frame_batch rows of md_C; n >= 1.  Queued on the stream: C is rewritten by the next call behind this one's readers.
int launch_mode_positions(msl_handle* h, long long n, int count, uint64_t seed, uint64_t first_frame, double* pos) {
    const int M = h->md_M, nb = h->md_nb;
    hipLaunchKernelGGL(mode_coefficients_kernel, dim3((unsigned)(((long long)M * count + 255) / 256)), dim3(256), 0, h->stream, h->md_tau, M,
                       count, (unsigned long long)seed, (unsigned long long)first_frame, h->md_dynamic ? 1 : 0, h->md_C);
    HIPCHK(h, hipGetLastError());
    auto launch = [&](auto kernel, int tile) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)((n + 255) / 256), (unsigned)((count + tile - 1) / tile)), dim3(256),
                           mode_positions_lds_bytes(nb, tile), h->stream, h->th_pos0, h->md_basis, h->md_q, h->md_C, h->md_W, n, nb, M, count, pos);
    };
    const bool lds = nb <= MODE_LDS_BASIS;
    if (count <= MODE_TILE_SMALL) {
        if (lds) launch(mode_positions_kernel<true, MODE_TILE_SMALL>, MODE_TILE_SMALL);
        else launch(mode_positions_kernel<false, MODE_TILE_SMALL>, MODE_TILE_SMALL);
    } else {
        if (lds) launch(mode_positions_kernel<true, MODE_TILE>, MODE_TILE);
        else launch(mode_positions_kernel<false, MODE_TILE>, MODE_TILE);
    }
    HIPCHK(h, hipGetLastError());
    return MSL_OK;
}

// stage_thermal for a group of phonon-mode frames
int stage_modes(msl_handle* h, const PotGroup& p, uint64_t seed, uint64_t first_frame, bool send_maps) {
    int rc;
    if (send_maps && (rc = stage_resident_maps(h, p))) return rc;
    return launch_mode_positions(h, p.n, p.g, seed, first_frame, h->d_pos);
}

int absorptive_tables(msl_handle* h, int nsp);

// Atoms of a group -> phase tables in sorted order: slice bins (atom_prep_kernel), stable counting sort with keys = frame x slice x
// species (bin_scan / bin_fill), the phase tables of both axes
int bin_atoms(msl_handle* h, const PotGroup& p) {
    const msl_config& c = h->cfg;
    const int nsp = p.nsp;
    HIPCHK(h, hipMemsetAsync(h->d_counts, 0, ((size_t)p.nkeys + 1) * sizeof(int), h->stream));
    const double lx = c.nx * c.dx, ly = c.ny * c.dy;
    // f_Z(q^2) depends on the grid and the species only (potentials.py:283-293 recomputes it per frame): build the table
    // when the species list changes, i.e. once per run
    if (nsp != h->ff_n || memcmp(p.species, h->ff_species, nsp * sizeof(int)) != 0 || (p.finite && h->ff_dz != c.dz)) {
        long long tot = (long long)c.nx * c.ny * nsp;
        if (p.finite) {                                  // the channel tables, once per (species list, grid, R, J, slab thickness)
            const long long tot_ch = (long long)c.nx * c.ny * p.ntab;
            hipLaunchKernelGGL(finite_formfactor_kernel, dim3((unsigned)((tot_ch + 255) / 256)), dim3(256), 0, h->stream, h->d_ff, h->d_abcd,
                               h->d_species, nsp, h->fin_R, h->fin_J, c.dz, c.nx, c.ny, 1.0 / lx, 1.0 / ly);
            h->ff_dz = c.dz;
        } else if (!h->abs_on)                           // (absorptive_tables writes f D there itself)
            hipLaunchKernelGGL(formfactor_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, h->stream, h->d_ff, h->d_abcd,
                               h->d_species, nsp, c.nx, c.ny, 1.0 / lx, 1.0 / ly);
        memcpy(h->ff_species, p.species, nsp * sizeof(int));
        h->ff_n = nsp;
        if (h->abs_on) { const int rc = absorptive_tables(h, nsp); if (rc) { h->ff_n = 0; return rc; } }
    }
    const long long atoms = (long long)p.n * p.g;
    if (p.finite) {
        // the slab lattice of the reference's slice rule: slab 0 = [c_0 - dz/2, c_0 + dz/2) although slice 0 counts atoms from lo[0] on
        const double dz = c.dz;
        const double e0 = c.nz > 1 ? h->h_lo[1] - dz : h->h_hi[0] - 1.5 * dz;
        hipLaunchKernelGGL(atom_prep_finite_kernel, dim3((unsigned)((atoms + 255) / 256)), dim3(256), 0, h->stream, h->d_pos, h->d_Z,
                           (long long)p.n, p.g, h->d_z2s, h->h_lo[0], h->h_hi[c.nz - 1], e0, dz / h->fin_J, c.nz, nsp, h->fin_R, h->fin_J,
                           p.ax1, p.ax2, p.axs, 1.0 / lx, 1.0 / ly, h->d_key, h->d_wgt, h->d_u1, h->d_u2, h->d_counts);
    } else
        hipLaunchKernelGGL(atom_prep_kernel, dim3((unsigned)((atoms + 255) / 256)), dim3(256), 0, h->stream, h->d_pos, h->d_Z,
                           (long long)p.n, p.g, h->d_z2s, h->d_lo, h->d_hi, c.nz, nsp, p.ax1, p.ax2, p.axs, 1.0 / lx, 1.0 / ly, h->d_key,
                           h->d_u1, h->d_u2, h->d_counts);
    hipLaunchKernelGGL(bin_scan_kernel, dim3(1), dim3(1024), 0, h->stream, h->d_counts, h->d_start, p.nkeys, p.sf_stream ? SF_ALIGN : 1);
    hipLaunchKernelGGL(bin_fill_kernel, dim3(p.nkeys), dim3(1024), 0, h->stream, h->d_key, (long long)p.n * p.rep, p.keys_per_frame, h->d_start, h->d_order);
    HIPCHK(h, hipGetLastError());
    // atoms that fell into a slice: d_start[nkeys], read by the kernels themselves (grids sized for all atoms of the group)
    const int* n_sorted = h->d_start + p.nkeys;
    if (p.rows_pad > 0x7fffffffLL) return fail(h, MSL_ERR_INVALID, "msl_build_potentials: %lld padded table rows in one group exceed 2^31", p.rows_pad);
    const long long tx = p.rows_pad * p.cx, ty = p.rows_pad * p.cy;
    if (p.finite)                                        // the weight of the partial atom rides on the x table alone
        hipLaunchKernelGGL(phase_table_weighted_kernel, dim3((unsigned)((tx + 255) / 256)), dim3(256), 0, h->stream, h->d_ex, h->d_u1,
                           h->d_wgt, h->d_order, n_sorted, c.nx, p.cx, p.cx);
    else
        hipLaunchKernelGGL(phase_table_kernel, dim3((unsigned)((tx + 255) / 256)), dim3(256), 0, h->stream, h->d_ex, h->d_u1,
                           h->d_order, n_sorted, c.nx, p.cx, p.cx);
    hipLaunchKernelGGL(phase_table_kernel, dim3((unsigned)((ty + 255) / 256)), dim3(256), 0, h->stream, h->d_ey, h->d_u2,
                       h->d_order, n_sorted, c.ny, p.cy, p.cy);
    return MSL_OK;
}

// Structure factors R_s of a group's slices into TR: matrix-core kernel over the quadrant of non-negative frequencies 0 .. n/2 in
// 32 x 32 tiles; on power-of-two grids (n/2 + 1 = 32 k + 1) the Nyquist row / column goes to the edge kernel instead of a tile row
// of its own
int launch_structure_factor(msl_handle* h, const PotGroup& p, const float* table = nullptr) {
    const msl_config& c = h->cfg;
    const float* ff = table ? table : h->d_ff.p;             // (the absorptive build runs it a second time, on d_ffa)
    const int cx = p.cx, cy = p.cy, nsp = p.ntab, n_slices = p.n_slices, full_rows = p.half_rows ? 0 : 1;     // (channel tables as species)
    const bool edge_x = (c.nx % 2 == 0) && (cx % 32 == 1) && cx > 1, edge_y = (c.ny % 2 == 0) && (cy % 32 == 1) && cy > 1;
    const int tiles_x = edge_x ? cx / 32 : (cx + 31) / 32, tiles_y = edge_y ? cy / 32 : (cy + 31) / 32;
    const int n_tiles = tiles_x * tiles_y, wg_per_slice = (n_tiles + 3) / 4;
    const long long n_wg = (long long)wg_per_slice * ((n_slices + 7) / 8 * 8);
    if (n_wg > 0x7fffffffLL) return fail(h, MSL_ERR_UNSUPPORTED, "structure factor: too many workgroups");
    if (p.sf_stream) {
        // persistent form, one wave per SIMD: one workgroup per CU, a multiple of 8 (XCD-local slices)
        const int n_pers = std::max(8, h->n_cus / 8 * 8);
        auto stream = [&](auto kernel, size_t lds, int tiles) {
            hipLaunchKernelGGL(kernel, dim3((unsigned)n_pers), dim3(256), lds, h->stream, p.TR, h->d_ex, h->d_ey, ff, h->d_start, nsp,
                               c.nx, c.ny, tiles_y, tiles, (int)p.rows_pad, full_rows, cx, cy, n_slices);
        };
        if (dbg_env("MSL_SF_F32"))                   // the exact-f32 matrix instruction (A/B against the split-bf16 form)
            stream(structure_factor_stream_kernel, 0, n_tiles);
        // two kx tiles per wave sharing the ey planes (potential.h) where a slice's tables outgrow an XCD's L2: 2048^2 x 50 potential
        // 8.67 -> 8.17 ms per frame, 1024^2 (C3) 3.72 -> 3.69 (kept on the one-tile kernel)
        else if ((n_tiles >= 512 || (tiles_x >= 2 && dbg_env("MSL_SF_TWO_TILES"))) && !dbg_env("MSL_SF_ONE_TILE"))
            stream(structure_factor_stream_bf16x2_kernel, 4 * 128 * 64 * sizeof(float), ((tiles_x + 1) / 2) * tiles_y);
        else
            stream(structure_factor_stream_bf16_kernel, 0, n_tiles);
    } else
        hipLaunchKernelGGL(structure_factor_quad_kernel, dim3((unsigned)n_wg), dim3(256), 0, h->stream, p.TR, h->d_ex, h->d_ey, ff,
                           h->d_start, nsp, c.nx, c.ny, tiles_y, n_tiles, (int)p.rows_pad, full_rows, cx, cy, n_slices, wg_per_slice);
    if (edge_x || edge_y) {
        const int bins = (edge_x ? cy : 0) + (edge_y ? (edge_x ? cx - 1 : cx) : 0);
        for (int s0 = 0; s0 < n_slices; s0 += 65535) {
            const int ns = std::min(65535, n_slices - s0);
            hipLaunchKernelGGL(structure_factor_edge_kernel, dim3((bins + 127) / 128, ns), dim3(128), 0, h->stream,
                               p.TR + (size_t)s0 * c.nx * c.ny, h->d_ex, h->d_ey, ff, h->d_start + (size_t)s0 * nsp, nsp, c.nx, c.ny,
                               edge_x ? 1 : 0, edge_y ? 1 : 0, full_rows, cx, cy);
        }
    }
    HIPCHK(h, hipGetLastError());
    return MSL_OK;
}

// One transposing pass of the potential's inverse transform along direction `o`, on the kernel of a PotIfft form; the LDS bytes and
// the lines per work item are the kernel's own (pot_ifft.h: Ifft*Lds).
template <typename Lds, typename Kernel>
int launch_ifft(msl_handle* h, Kernel kernel, int per_cu, const IfftJob& j) {
    const long long items = (long long)((j.n_lines + Lds::LINES - 1) / Lds::LINES) * j.n_images;
    const long long slots = (long long)h->n_cus * std::max(1, std::min(per_cu, (int)((size_t)h->lds_limit / Lds::bytes)));
    return launch_lds(h, kernel, dim3((unsigned)std::min(items, slots)), dim3(Lds::NT), Lds::bytes, K_OTHER, j);
}

// 2048-point lines, one wave per line (fft2048_wave)
int launch_ifftTW(msl_handle* h, const msl_handle::OpDir& o, IfftJob j) {
    j.tw = o.tw; j.tw2 = o.tw2; j.n_line = IfftTWLds::N;
    return launch_ifft<IfftTWLds>(h, ifftTW_kernel, 1, j);
}

// lines of any length up to 1024 by chirp-z on the register FFTs (o.cz)
int launch_ifftTB(msl_handle* h, const msl_handle::OpDir& o, IfftJob j) {
    const CzTables& t = o.cz;
    j.tw = t.tw; j.tw2 = t.tw2; j.bf = t.bf; j.bw = t.bw;
    if (t.R == 64) return launch_ifft<IfftTB2Lds>(h, ifftTB2_kernel, 1, j);      // 513 .. 1024 points: the wave-per-line 2048-point FFT
    if (t.R == 16) return launch_ifft<IfftTBLds<16>>(h, ifftTB_kernel<16>, 4, j);
    // first pass (no epilogue): two lines per group and tile round
    if (!j.potential && !dbg_env("MSL_NO_TWO_LINE_IFFT")) return launch_ifft<IfftTBTwoLds>(h, ifftTB_two_kernel, 1, j);
    // second pass on a half spectrum: two real lines per transform (32-line work items)
    if (j.herm && j.potential && !dbg_env("MSL_NO_PAIRED_IFFT")) return launch_ifft<IfftTBLds<32, true>>(h, ifftTB_kernel<32, true>, 1, j);
    return launch_ifft<IfftTBLds<32>>(h, ifftTB_kernel<32>, 1, j);
}

// lines of 2 R^2 = 512 points
int launch_ifftT2(msl_handle* h, const msl_handle::OpDir& o, IfftJob j) {
    j.tw = o.tw; j.tw2 = o.tw2; j.n_line = IfftT2Lds<16>::N;
    // second pass on a half spectrum: two real lines per transform (32-line work items)
    if (j.herm && j.potential && j.n_lines % 32 == 0 && !dbg_env("MSL_NO_PAIRED_IFFT"))
        return launch_ifft<IfftT2Lds<16, true>>(h, ifftT2_kernel<16, true>, 2, j);
    return launch_ifft<IfftT2Lds<16>>(h, ifftT2_kernel<16>, 2, j);
}

// The transposing forms: TR -> TRT along y on the rows kx <= nx/2 (the others are their mirror images, taken by the second pass's
// loads) in whole blocks of `line_block` lines (the surplus rows are never read), then TRT -> TR / TRT along x with the potential
// epilogue: the slices a pass along x reads stay in TRT as rows.
int ifft_transposed(msl_handle* h, const PotGroup& p, int line_block, int (*launch)(msl_handle*, const msl_handle::OpDir&, IfftJob)) {
    const msl_config& c = h->cfg;
    const long long npix = (long long)c.nx * c.ny;
    IfftJob a{};
    a.in = p.TR; a.out_t = p.TRT; a.out_rows = nullptr;
    a.in_is = a.out_t_is = npix; a.in_pitch = c.ny; a.out_t_pitch = c.nx; a.n_images = p.n_slices;
    a.n_lines = (c.nx / 2 + 1 + line_block - 1) / line_block * line_block; a.n_line = c.ny;
    a.potential = 0; a.rows_parity = -1; a.slice_mod = c.nz;
    IfftJob b{};
    b.in = p.TRT; b.out_t = p.TR; b.out_rows = p.TRT;
    b.in_is = b.out_t_is = b.out_rows_is = npix; b.in_pitch = c.nx; b.out_t_pitch = c.ny; b.out_rows_pitch = c.nx;
    b.n_lines = c.ny; b.n_line = c.nx; b.n_images = p.n_slices; b.potential = 1; b.herm = 1; b.slice_mod = c.nz;
    b.rows_parity = slice_is_transposed(h, 1) ? 1 : 0;       // (scheme b: slice s is read along x iff s is odd)
    // the epilogue takes sincospi(sigma_over_pi * (x * scale)): the two constants are multiplied in double here and rounded once (x * 1
    // is exact), instead of two rounded constants and two rounded products -- at a pixel with a phase of tens of radians each of
    // them is 2^-24 of the phase (white-potential parity, 2048 x 2048 x 3: E_pix 4.69e-5 with the constants apart)
    b.scale = 1.0f;
    b.sigma_over_pi = (float)(1.0 / ((double)c.nx * c.ny) / (c.dx * c.dx * c.dy * c.dy) * (c.sigma / M_PI));
    const int rc = launch(h, h->opy, a);
    return rc ? rc : launch(h, h->opx, b);
}

// PI_LINES: rows, then columns with the epilogue, in place; slices a pass along x reads are transposed by the column kernel (COL_TPOT) or afterwards
int ifft_inplace(msl_handle* h, const PotGroup& p) {
    const msl_config& c = h->cfg;
    int rc;
    if (h->Ry) {
        RowJob r = row_job(h, p.TR, p.n_slices, c.ny);
        r.do_ifft = 1;
        if (p.half_rows) { const int Gr = 256 / h->Ry; r.nx = (c.nx / 2 + 1 + Gr - 1) / Gr * Gr; }     // whole row groups (the surplus rows are never read)
        if ((rc = launch_row_fast(h, r, K_OTHER))) return rc;
    } else {
        LineArgs r = row_args(h, p.TR, p.TR, p.n_slices, c.ny);
        r.fft1 = -1;
        if ((rc = launch_lines(h, h->plan_y, r, K_OTHER))) return rc;
    }
    if (h->Rx) {
        ColJob k = col_job(h, p.TR, p.TR, p.n_slices, c.ny, c.ny);
        k.flags = COL_INV | COL_POTENTIAL; k.scale = p.vscale; k.sigma = (float)c.sigma; k.out_real = h->V; k.slice_mod = c.nz;
        // (a kept V is written by the untransposed store only: with keep_potential the x-pass slices are transposed afterwards)
        if (h->onepass && !h->V) { k.flags |= COL_TPOT; k.tparity = h->scheme_b ? 0 : ((c.nz - 1) & 1); k.out_t = p.TRT; }
        if ((rc = p.half_rows ? launch_col_herm(h, k, K_OTHER) : launch_col_fast(h, k, K_OTHER))) return rc;
        return (h->onepass && h->V) ? transpose_odd_slices(h, p.slot) : MSL_OK;
    }
    LineArgs k = col_args(h, p.TR, p.TR, p.n_slices, c.ny, c.ny);
    k.fft1 = -1; k.scale = p.vscale;
    k.store_mode = STORE_POTENTIAL; k.out_real = h->V; k.sigma = (float)c.sigma;
    if ((rc = launch_lines(h, h->plan_x, k, K_OTHER))) return rc;
    for (int f = 0; f < p.g && rc == MSL_OK; ++f) rc = transpose_odd_slices(h, p.slot + f);     // one-pass loop on such a grid: x-pass slices transposed, stack by stack
    return rc;
}

// V_s = Re ifft2(R_s) / (dx^2 dy^2);  t_s = exp(i sigma V_s)  -- in place over the (frames, nz, nx, ny) stacks of the group.
// Slices a pass along x reads are kept transposed (scheme b: odd slices; alternating scheme: odd distance to the last one):
// with several frames per launch the slice number is the image index modulo nz (slice_mod).
int potential_ifft(msl_handle* h, const PotGroup& p) {
    h->cur = nullptr;
    switch (h->pot_ifft) {
    case PI_WAVE2K: return ifft_transposed(h, p, IfftTWLds::LINE_BLOCK, launch_ifftTW);
    case PI_CHIRPZ: return ifft_transposed(h, p, IfftTBLds<32>::LINE_BLOCK, launch_ifftTB);
    case PI_TWO:    return ifft_transposed(h, p, IfftT2Lds<16>::LINE_BLOCK, launch_ifftT2);
    default:        return ifft_inplace(h, p);
    }
}

// ---- absorptive potential (absorptive.h) ----
// The tables of the species in d_species, once per species list, grid or set of widths: d_ff = f D and, with absorption, d_ffa = g.
// Four transforms of fft2_inplace over all species at once with the pointwise kernels between them; the work array lives for this
// call only (the call waits for the stream: once per run).
int absorptive_tables(msl_handle* h, int nsp) {
    const msl_config& c = h->cfg;
    const long long npix = (long long)c.nx * c.ny, tot = npix * nsp;
    const double inv_lx = 1.0 / (c.nx * c.dx), inv_ly = 1.0 / (c.ny * c.dy), cell = c.dx * c.dx * c.dy * c.dy;
    const dim3 grid((unsigned)((tot + 255) / 256)), block(256);
    DevBuf<float2> W, F0, W0;           // F0 = f + i f D and W0 = V1 + i Vbar1 are kept for the detector tables only
    DevBuf<float> vb;
    int rc;
    if (h->abs_absorb && ((rc = W.alloc(h, (size_t)tot)) || (rc = h->d_ffa.reserve(h, (size_t)tot)))) return rc;
    if (h->tds_on && ((rc = F0.alloc(h, (size_t)tot)) || (rc = W0.alloc(h, (size_t)tot)) || (rc = vb.alloc(h, (size_t)tot)) ||
                      (rc = h->tds_g.reserve(h, (size_t)tot * h->tds_n)))) return rc;
    hipLaunchKernelGGL(absorptive_formfactor_kernel, grid, block, 0, h->stream, h->d_ff, W.p, h->d_abcd, h->d_abs_u, h->d_species, nsp,
                       c.nx, c.ny, inv_lx, inv_ly);
    HIPCHK(h, hipGetLastError());
    if (!h->abs_absorb) return MSL_OK;
    h->cur = nullptr;
    if (h->tds_on) HIPCHK(h, hipMemcpyAsync(F0, W, (size_t)tot * sizeof(float2), hipMemcpyDeviceToDevice, h->stream));
    if ((rc = fft2_inplace(h, W, nsp, -1, (float)(1.0 / (double)npix / cell), c.ny))) return rc;          // V1 + i Vbar1
    if (h->tds_on) HIPCHK(h, hipMemcpyAsync(W0, W, (size_t)tot * sizeof(float2), hipMemcpyDeviceToDevice, h->stream));
    hipLaunchKernelGGL(absorptive_square_kernel, grid, block, 0, h->stream, W.p, h->d_ffa, tot);
    if ((rc = fft2_inplace(h, W, nsp, +1, 1.0f, c.ny))) return rc;
    hipLaunchKernelGGL(absorptive_damp_kernel, grid, block, 0, h->stream, W.p, h->d_abs_u, h->d_species, nsp, c.nx, c.ny, inv_lx, inv_ly);
    if ((rc = fft2_inplace(h, W, nsp, -1, (float)(1.0 / (double)npix), c.ny))) return rc;                 // <V1^2>
    hipLaunchKernelGGL(absorptive_variance_kernel, grid, block, 0, h->stream, W.p, h->d_ffa, tot);
    if ((rc = fft2_inplace(h, W, nsp, +1, 1.0f, c.ny))) return rc;
    hipLaunchKernelGGL(absorptive_real_kernel, grid, block, 0, h->stream, h->d_ffa, W.p, tot, (float)cell);
    HIPCHK(h, hipGetLastError());
    // the detector tables g_det (tds.h): the same four transforms per detector, on M_d (f + i f D) and the products with V1, Vbar1
    for (int d = 0; h->tds_on && d < h->tds_n; ++d) {
        hipLaunchKernelGGL(tds_mask_kernel, grid, block, 0, h->stream, W.p, F0.p, h->tds_bits.p, d, npix, tot);
        if ((rc = fft2_inplace(h, W, nsp, -1, (float)(1.0 / (double)npix / cell), c.ny))) return rc;      // V1M + i Vbar1M
        hipLaunchKernelGGL(tds_product_kernel, grid, block, 0, h->stream, W.p, W0.p, vb.p, tot);
        if ((rc = fft2_inplace(h, W, nsp, +1, 1.0f, c.ny))) return rc;
        hipLaunchKernelGGL(absorptive_damp_kernel, grid, block, 0, h->stream, W.p, h->d_abs_u, h->d_species, nsp, c.nx, c.ny, inv_lx, inv_ly);
        if ((rc = fft2_inplace(h, W, nsp, -1, (float)(1.0 / (double)npix), c.ny))) return rc;
        hipLaunchKernelGGL(absorptive_variance_kernel, grid, block, 0, h->stream, W.p, vb.p, tot);
        if ((rc = fft2_inplace(h, W, nsp, +1, 1.0f, c.ny))) return rc;
        hipLaunchKernelGGL(absorptive_real_kernel, grid, block, 0, h->stream, h->tds_g + (size_t)d * tot, W.p, tot, (float)cell);
        HIPCHK(h, hipGetLastError());
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));             // W is freed on return
    return MSL_OK;
}

// ifft_inplace's two passes with the real store into `out_real` (the stacks of the group, natural order) and no transposed slices;
// the t it leaves in TR (sigma = 0) is overwritten by the absorptive epilogue
int absorptive_ifft(msl_handle* h, const PotGroup& p, float* out_real) {
    const msl_config& c = h->cfg;
    int rc;
    if (h->Ry) {
        RowJob r = row_job(h, p.TR, p.n_slices, c.ny);
        r.do_ifft = 1;
        if (p.half_rows) { const int Gr = 256 / h->Ry; r.nx = (c.nx / 2 + 1 + Gr - 1) / Gr * Gr; }
        if ((rc = launch_row_fast(h, r, K_OTHER))) return rc;
    } else {
        LineArgs r = row_args(h, p.TR, p.TR, p.n_slices, c.ny);
        r.fft1 = -1;
        if ((rc = launch_lines(h, h->plan_y, r, K_OTHER))) return rc;
    }
    if (h->Rx) {
        ColJob k = col_job(h, p.TR, p.TR, p.n_slices, c.ny, c.ny);
        k.flags = COL_INV | COL_POTENTIAL; k.scale = p.vscale; k.sigma = 0.f; k.out_real = out_real; k.slice_mod = c.nz;
        return p.half_rows ? launch_col_herm(h, k, K_OTHER) : launch_col_fast(h, k, K_OTHER);
    }
    LineArgs k = col_args(h, p.TR, p.TR, p.n_slices, c.ny, c.ny);
    k.fft1 = -1; k.scale = p.vscale;
    k.store_mode = STORE_POTENTIAL; k.out_real = out_real; k.sigma = 0.f;
    return launch_lines(h, h->plan_x, k, K_OTHER);
}

// ---- element maps: the weight stack (ionization.h) ----
// The tables of the channels, (ion_n, n_species, nx, ny): made when the species list of a build is not the one they were made for
// (msl_set_ionization forgets it).  Each is non-zero for the species of its channel only, so the structure factor of the build sums
// the atoms of that element and no others, in the slices its own sort has put them in.
int ion_tables(msl_handle* h, const PotGroup& p) {
    const msl_config& c = h->cfg;
    if (p.nsp == h->ion_nsp && memcmp(p.species, h->ion_species, p.nsp * sizeof(int)) == 0) return MSL_OK;
    const long long tot = (long long)c.nx * c.ny * p.nsp;
    h->ion_nsp = 0;
    const int rc = h->ion_tab.reserve(h, (size_t)tot * h->ion_n);
    if (rc) return rc;
    for (int e = 0; e < h->ion_n; ++e)
        hipLaunchKernelGGL(ion_table_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, h->stream, h->ion_tab + (size_t)e * tot, p.nsp,
                           p.z2s[h->ion_Z[e]], c.nx, c.ny, 1.0 / (c.nx * c.dx), 1.0 / (c.ny * c.dy), h->ion_width[e], h->ion_cross[e] * c.dx * c.dy);
    HIPCHK(h, hipGetLastError());
    memcpy(h->ion_species, p.species, p.nsp * sizeof(int));
    h->ion_nsp = p.nsp;
    return MSL_OK;
}

// The weight stack of a group whose atoms bin_atoms has sorted (`atoms` false: none, the stack is zero), before the potential of the
// group is made: per channel the structure factor with the channel's table and absorptive_ifft's two passes into ion_W, through the
// group's own transmission slot, which the build overwrites afterwards.  A channel whose element the structure does not hold is zero.
int ionization_group(msl_handle* h, const PotGroup& p, bool atoms) {
    const msl_config& c = h->cfg;
    const size_t npix = (size_t)c.nx * c.ny, stack = npix * c.nz;
    if (p.g != 1 || p.finite || h->pot_ifft != PI_LINES)
        return fail(h, MSL_ERR_UNSUPPORTED, "ionization: the weight stack is that of one frame, built on the two-pass loop without finite projection");
    int rc;
    h->cur = nullptr;
    if (!h->ion_W && (rc = h->ion_W.alloc(h, stack * h->ion_n))) return rc;
    if (atoms && (rc = ion_tables(h, p))) return rc;
    for (int e = 0; e < h->ion_n; ++e) {
        float* W = h->ion_W + (size_t)e * stack;
        if (!atoms || p.z2s[h->ion_Z[e]] < 0) {
            HIPCHK(h, hipMemsetAsync(W, 0, stack * sizeof(float), h->stream));
            continue;
        }
        if ((rc = launch_structure_factor(h, p, h->ion_tab + (size_t)e * npix * p.nsp)) || (rc = absorptive_ifft(h, p, W))) return rc;
    }
    return MSL_OK;
}

// t = exp(i sigma Vbar - sigma^2 Omega) of the stacks in the batch slots slot .. slot + count - 1, from abs_V / abs_O into trans
// (natural order), with the handle's current sigma
int absorptive_transmission(msl_handle* h, int slot, int count) {
    const msl_config& c = h->cfg;
    const size_t stack = (size_t)c.nx * c.ny * c.nz, off = (size_t)slot * stack;
    const long long n = (long long)(stack * count);
    float2* t = h->trans + off;
    const float* V = h->abs_V + off;
    const float* Om = h->abs_absorb ? h->abs_O + off : nullptr;
    const bool vec = (((uintptr_t)t | (uintptr_t)V | (uintptr_t)Om) & 15) == 0;
    const float sop = (float)(c.sigma / M_PI), s2 = (float)(c.sigma * c.sigma);
    const dim3 grid((unsigned)((n + 1023) / 1024)), block(256);
    if (n > 0x7fffffffLL * 1024) return fail(h, MSL_ERR_UNSUPPORTED, "absorptive transmission: too many pixels");
    if (Om) {
        if (vec) hipLaunchKernelGGL((transmission_absorptive_kernel<true, true>), grid, block, 0, h->stream, t, V, Om, n, sop, s2);
        else hipLaunchKernelGGL((transmission_absorptive_kernel<true, false>), grid, block, 0, h->stream, t, V, Om, n, sop, s2);
    } else {
        if (vec) hipLaunchKernelGGL((transmission_absorptive_kernel<false, true>), grid, block, 0, h->stream, t, V, Om, n, sop, s2);
        else hipLaunchKernelGGL((transmission_absorptive_kernel<false, false>), grid, block, 0, h->stream, t, V, Om, n, sop, s2);
    }
    HIPCHK(h, hipGetLastError());
    return MSL_OK;
}

// The TDS weight stack in place (tds_weight_kernel): from Omega_det with the handle's sigma (from_omega), or from the weights of the
// beam it was made with (msl_set_beam)
int tds_weights(msl_handle* h, bool from_omega) {
    const msl_config& c = h->cfg;
    const long long n = (long long)c.nx * c.ny * c.nz * h->tds_n;
    const double a = 2.0 * c.sigma * c.sigma, a_old = 2.0 * h->tds_sigma * h->tds_sigma;
    if (!from_omega && a_old == 0.0) {
        if (a == 0.0) return MSL_OK;
        return fail(h, MSL_ERR_STATE, "msl_set_beam: the TDS weights were made at sigma = 0 and hold nothing to remake; rebuild the potential");
    }
    hipLaunchKernelGGL(tds_weight_kernel, dim3((unsigned)((n + 1023) / 1024)), dim3(256), 0, h->stream, h->tds_W.p, n, (float)a,
                       from_omega ? 0.f : (float)(a / a_old));
    HIPCHK(h, hipGetLastError());
    h->tds_sigma = c.sigma;
    return MSL_OK;
}

// The absorptive build of a group whose atoms bin_atoms has sorted (`atoms` false: none, both stacks are zero): the structure factor
// and the inverse transform twice, with d_ff into Vbar and with d_ffa into Omega, then the epilogue and the transposed copies of the
// slices the one-pass loop reads along x.  With TDS on, once more per detector with its table g_det into the weight stack.
int absorptive_group(msl_handle* h, const PotGroup& p, bool atoms) {
    const msl_config& c = h->cfg;
    const size_t stack = (size_t)c.nx * c.ny * c.nz, off = (size_t)p.slot * stack;
    int rc;
    h->cur = nullptr;
    if (h->tds_on && !h->tds_W && (rc = h->tds_W.alloc(h, stack * h->tds_n))) return rc;
    if (!atoms) {
        HIPCHK(h, hipMemsetAsync(h->abs_V + off, 0, stack * p.g * sizeof(float), h->stream));
        if (h->abs_absorb) HIPCHK(h, hipMemsetAsync(h->abs_O + off, 0, stack * p.g * sizeof(float), h->stream));
        if (h->tds_on) HIPCHK(h, hipMemsetAsync(h->tds_W, 0, stack * h->tds_n * sizeof(float), h->stream));
    } else {
        if ((rc = launch_structure_factor(h, p)) || (rc = absorptive_ifft(h, p, h->abs_V + off))) return rc;
        if (h->abs_absorb && ((rc = launch_structure_factor(h, p, h->d_ffa)) || (rc = absorptive_ifft(h, p, h->abs_O + off)))) return rc;
        for (int d = 0; h->tds_on && d < h->tds_n; ++d)
            if ((rc = launch_structure_factor(h, p, h->tds_g + (size_t)d * c.nx * c.ny * p.nsp)) ||
                (rc = absorptive_ifft(h, p, h->tds_W + (size_t)d * stack))) return rc;
    }
    if (h->tds_on && (rc = tds_weights(h, true))) return rc;
    if ((rc = absorptive_transmission(h, p.slot, p.g))) return rc;
    for (int f = 0; f < p.g && rc == MSL_OK; ++f) rc = transpose_odd_slices(h, p.slot + f);
    return rc;
}

// ---- band-limited transmission functions (bandlimit.h) ----
// t <- B_x B_y t of the `count` stacks from batch slot `slot` on, in place in `trans` in natural order: along each axis one launch of
// the generic line kernel, forward transform, x mask / n, inverse transform -- the column step of the two-pass slice loop with the
// mask in the place of the Fresnel table.  Queued on the stream, no host copy.
int bandlimit_lowpass(msl_handle* h, int slot, int count) {
    const msl_config& c = h->cfg;
    float2* t = h->trans + (size_t)slot * c.nz * c.nx * c.ny;
    const long long images = (long long)c.nz * count;
    if (images > 0x7fffffff) return fail(h, MSL_ERR_UNSUPPORTED, "band limit: too many slices");
    h->cur = nullptr;
    LineArgs r = row_args(h, t, t, (int)images, c.ny);
    r.fft1 = +1; r.m1_kind = MUL_VEC; r.m1 = h->bl_my; r.fft2 = -1;
    int rc = launch_lines(h, h->plan_y, r, K_OTHER);
    if (rc) return rc;
    LineArgs k = col_args(h, t, t, (int)images, c.ny, c.ny);
    k.fft1 = +1; k.m1_kind = MUL_VEC; k.m1 = h->bl_mx; k.fft2 = -1;
    return launch_lines(h, h->plan_x, k, K_OTHER);
}

// ==== handle settings: what each setter re-derives ============================
// One function per derived state -- refresh_propagator, set_loop_mode(allowed_onepass), remake_transmission / drop_potential,
// drop_smatrix_result -- and the five setters, each of which changes its setting and calls those.

// ---- propagator tables ----
// float64 cos and sin of sign * pi lambda dz k^2 at the n frequencies of an axis of spacing d, in FFT order
void host_phase_table(const msl_config& c, int n, double d, double sign, std::vector<double>& re, std::vector<double>& im) {
    re.resize(n); im.resize(n);
    for (int m = 0; m < n; ++m) {
        const int f = (m < (n + 1) / 2) ? m : m - n;
        const double k = f * (1.0 / (n * d));
        const double ph = sign * M_PI * c.wavelength * c.dz * k * k;
        re[m] = cos(ph); im[m] = sin(ph);
    }
}

// Filter of the convolution that is the propagation along a convolution axis (conv_len) of n points, from its float64 table P = pr + i pi:
// a = ifft_n(P) (float64), wrapped to the cyclic length M, filter = FFT_M(a) / M, stored as its first half + 1 (NH + 2 entries,
// rowTB / rowTB2), or for M = 4096 in the split order of rowTC2_pass_kernel (even entries 0..1024, odd entries from 1026)
int fill_conv_filter(msl_handle* h, const msl_handle::OpDir& o, const std::vector<double>& pr, const std::vector<double>& pi) {
    const int n = o.n, M = conv_len(o), NH = M / 2;
    std::vector<double> er(n), ei(n), qr(M, 0.0), qi(M, 0.0);
    for (int m = 0; m < n; ++m) {
        const double a = 2.0 * M_PI * (double)m / (double)n;
        er[m] = cos(a); ei[m] = sin(a);
    }
    for (int j = 0; j < n; ++j) {                      // a[j] = (1/n) sum_m P[m] e^{+2 pi i m j / n}
        double sr = 0.0, si = 0.0;
        long long t = 0;
        for (int m = 0; m < n; ++m) {
            sr += pr[m] * er[t] - pi[m] * ei[t];
            si += pr[m] * ei[t] + pi[m] * er[t];
            t += j; if (t >= n) t -= n;
        }
        sr /= n; si /= n;
        qr[j] = sr; qi[j] = si;                         // lag +j
        if (j) { qr[M - n + j] = sr; qi[M - n + j] = si; }   // lag j - n  (M - (n - j))
    }
    host_fft_pow2(qr, qi);
    std::vector<float2> qf(conv_filter_entries(o), make_float2(0.f, 0.f));
    if (o.base == AX_CONV4K) {
        for (int k = 0; k <= 1024; ++k) qf[k] = make_float2((float)(qr[2 * k] / M), (float)(qi[2 * k] / M));
        for (int k = 0; k < 1024; ++k) qf[1026 + k] = make_float2((float)(qr[2 * k + 1] / M), (float)(qi[2 * k + 1] / M));
    } else {
        for (int j = 0; j <= NH; ++j) qf[j] = make_float2((float)(qr[j] / M), (float)(qi[j] / M));
    }
    return copy_table(h, o.qf, qf);
}

// Fresnel propagator, separable: P[kx,ky] = exp(-i pi lambda dz kx^2) * exp(-i pi lambda dz ky^2) (multislice.py:273-275), written on
// the host, axis by axis: the plain table, the layer tap's conjugate, and from the plain table's values the split-order copy of a
// 2R^2 axis and the filter of a convolution axis
int fill_propagator(msl_handle* h) {
    const msl_config& c = h->cfg;
    std::vector<double> re, im, cr, ci;
    int rc;
    for (int a = 0; a < 2; ++a) {
        const msl_handle::OpDir& o = a ? h->opy : h->opx;
        const int n = a ? c.ny : c.nx;
        const double d = a ? c.dy : c.dx;
        std::vector<float2> plain(n), conj(n), split(n);
        host_phase_table(c, n, d, -1.0, re, im);
        host_phase_table(c, n, d, +1.0, cr, ci);
        for (int m = 0; m < n; ++m) {
            plain[m] = make_float2((float)(re[m] / n), (float)(im[m] / n));      // with the 1/n of the inverse FFT folded in
            conj[m] = make_float2((float)cr[m], (float)ci[m]);                    // exp(+i pi lambda dz k^2), unscaled
        }
        for (int b = 0; b < 2; ++b)                                               // entry [b*R^2 + k] = P[2k + b]
            for (int k = 0; k < n / 2; ++k) split[b * (n / 2) + k] = plain[2 * k + b];
        if ((rc = copy_table(h, a ? h->pyt : h->pxt, plain)) || (rc = copy_table(h, a ? h->tap_cy : h->tap_cx, conj)) ||
            (o.base == AX_TWO && (rc = copy_table(h, o.ptab, split))) || (conv_len(o) && (rc = fill_conv_filter(h, o, re, im)))) return rc;
    }
    return MSL_OK;
}

// The same tables with the tilt factor exp(-2 pi i dz tan(theta) k) and the mask of the band limit, written by the kernels of
// propagator.h on the handle's stream: no host table, no copy and no wait, so a change is ordered behind the passes queued before it.
int fill_propagator_device(msl_handle* h) {
    const msl_config& c = h->cfg;
    size_t work = 0;                                        // float64 entries of the convolution sums: P, E (n each), q, W (M each)
    for (const msl_handle::OpDir* o : {&h->opx, &h->opy})
        if (conv_len(*o)) work = std::max(work, 2 * (size_t)o->n + 2 * (size_t)conv_len(*o));
    int rc = h->tilt_work.reserve(h, work);
    if (rc) return rc;
    for (int axis = 0; axis < 2; ++axis) {
        const msl_handle::OpDir& o = axis ? h->opy : h->opx;
        const int n = axis ? c.ny : c.nx, M = conv_len(o);
        const double d = axis ? c.dy : c.dx;
        // the half-spectrum layout holds the filter of an even table only, and no pass reads qf under a tilted axis (set_loop_mode has
        // the two-pass loop on, a mixed axis reads the plain table): the filter is written at a zero tangent, which every way back to
        // the convolution pass goes through (msl_set_tilt with 0 along the axis)
        const bool filter = M && h->set.tilt_tan[axis] == 0.0;
        double2* Pd = filter ? (double2*)h->tilt_work : nullptr;
        double2* Ed = filter ? Pd + n : nullptr;
        double2* q = filter ? Ed + n : nullptr;
        double2* Wd = filter ? q + M : nullptr;
        float2* split = o.base == AX_TWO ? (float2*)o.ptab : nullptr;
        const int lanes = filter ? std::max(n, M) : n;
        hipLaunchKernelGGL(propagator_tables_kernel, dim3((unsigned)((lanes + PROP_BLOCK - 1) / PROP_BLOCK)), dim3(PROP_BLOCK), 0, h->stream,
                           n, M, 1.0 / (n * d), 0.5 * c.wavelength * c.dz, c.dz * h->set.tilt_tan[axis], axis ? h->pyt : h->pxt, split,
                           axis ? h->tap_cy : h->tap_cx, Pd, Ed, Wd);
        HIPCHK(h, hipGetLastError());
        if (h->set.bl_on) {                                     // the band limit: before the filter sums, which then see the masked table
            hipLaunchKernelGGL(propagator_bandlimit_kernel, dim3((unsigned)((n + PROP_BLOCK - 1) / PROP_BLOCK)), dim3(PROP_BLOCK), 0, h->stream,
                               n, h->set.bl_cut[axis], axis ? h->pyt : h->pxt, split, axis ? h->tap_cy : h->tap_cx, Pd);
            HIPCHK(h, hipGetLastError());
        }
        if (!filter) continue;
        const int gap = M - 2 * n + 1, entries = (int)conv_filter_entries(o);
        hipLaunchKernelGGL(conv_lag_kernel, dim3((unsigned)(n + (gap + PROP_BLOCK - 1) / PROP_BLOCK)), dim3(PROP_BLOCK), 0, h->stream, n, M,
                           Pd, Ed, q);
        HIPCHK(h, hipGetLastError());
        hipLaunchKernelGGL(conv_filter_kernel, dim3((unsigned)entries), dim3(PROP_BLOCK), 0, h->stream, n, M, entries,
                           o.base == AX_CONV4K ? 1 : 0, q, Wd, (float2*)o.qf);
        HIPCHK(h, hipGetLastError());
    }
    return MSL_OK;
}

// The only caller of the two fillers and the only place that chooses between them.  A handle on which msl_set_tilt was never called
// and which has no band limit runs on the host tables, every other one on the device tables (equal up to one float rounding per
// entry).  The rule is there for the way back: a run without either setting, and one whose limit was set and cleared again, give bit
// for bit what they gave before the settings existed (test_untilted_outputs_unchanged, test_off_is_off, tests/test_gpu_settings_order.py).
int refresh_propagator(msl_handle* h) { return (h->set.tilt_set || h->set.bl_on) ? fill_propagator_device(h) : fill_propagator(h); }

// ---- loop mode ----
// The convolution passes keep the first half of their filter and mirror the rest (Q[M - k] = Q[k]), and the 2048-point wave kernel
// reads its Fresnel factors the same way: both hold for an even table only, which a tilted axis does not have.  The direct kernels
// (four-step, 2 R^2, mixed radix) read whole tables and take any tilt; so does the two-pass loop, on the plain tables.
bool tilt_needs_two_pass(const msl_handle* h, double tan_x, double tan_y) {
    auto even_only = [](const msl_handle::OpDir& o) { return o.kind == AX_CONV || o.kind == AX_CONV2K || o.kind == AX_CONV4K || o.kind == AX_WAVE2K; };
    return (tan_x != 0.0 && even_only(h->opx)) || (tan_y != 0.0 && even_only(h->opy));
}

// The loop a handle may run under the tangents (tan_x, tan_y): the one msl_create planned, unless the TDS signal, the ionisation signal,
// the adjoint (slice_loop takes them on the two-pass loop only) or the tilt asks for the two-pass loop
bool allowed_onepass(const msl_handle* h, double tan_x, double tan_y) {
    return h->onepass_planned && !h->tds_on && !h->ion_on && !h->adj_on && !tilt_needs_two_pass(h, tan_x, tan_y);
}

// Switch a handle planned for the one-pass loop to the two-pass loop and back, on the stream.  The two-pass loop and the potential
// build next to it (PI_LINES, untransposed stores) read and write `trans` in natural order only; the one-pass loop keeps every second
// slice transposed in transT.  The stacks a potential build has filled are carried over, every batch slot.
int set_loop_mode(msl_handle* h, bool onepass) {
    if (onepass == h->onepass) return MSL_OK;
    int rc = MSL_OK;
    for (int f = 0; !onepass && h->have_potential && f < h->FB && rc == MSL_OK; ++f) rc = restore_natural_slices(h, f);
    if (rc) return rc;
    h->onepass = onepass;
    h->pot_ifft = onepass ? plan_pot_ifft(h) : PI_LINES;
    for (int f = 0; onepass && h->have_potential && f < h->FB && rc == MSL_OK; ++f) rc = transpose_odd_slices(h, f);
    return rc;
}

// ---- transmission stacks ----
// t = exp(i sigma V) of one stack with the handle's sigma, from V (nz, nx, ny) into batch slot `slot` in natural order
int transmission_from_V(msl_handle* h, const float* V, int slot) {
    const size_t n = (size_t)h->cfg.nx * h->cfg.ny * h->cfg.nz;
    hipLaunchKernelGGL(transmission_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, h->trans + (size_t)slot * n, V,
                       (long long)n, (float)h->cfg.sigma);
    HIPCHK(h, hipGetLastError());
    return MSL_OK;
}

// What `count` stacks just written in natural order from batch slot `slot` on still need: the low-pass while a band limit is on, and
// the transposed copies of the slices the one-pass loop reads along x
int finish_stacks(msl_handle* h, int slot, int count) {
    int rc = h->set.bl_on ? bandlimit_lowpass(h, slot, count) : MSL_OK;
    for (int f = 0; f < count && rc == MSL_OK; ++f) rc = transpose_odd_slices(h, slot + f);
    return rc;
}

// The low-pass of stacks a build has left in the order of the slice loop (build_potentials, while a band limit is on): the transposed
// slices come back to natural order first (a no-op on the two-pass loop), so the stack is limited once, in one orientation
int bandlimit_built(msl_handle* h, int slot, int count) {
    int rc = MSL_OK;
    for (int f = 0; f < count && rc == MSL_OK; ++f) rc = restore_natural_slices(h, slot + f);
    return rc ? rc : finish_stacks(h, slot, count);
}

// The stacks again from what is resident, with the handle's sigma and under its limit: from the two absorptive stacks, every batch slot
// (and the TDS weights, which carry 2 sigma^2, from themselves), or else from the kept V (keep_potential runs at a frame batch of 1:
// one stack, slot 0).  The caller has checked that one of the two is there.  Waits for the stream.
int remake_transmission(msl_handle* h) {
    int rc;
    if (h->abs_built) {
        // finish_stacks with the weights between its two steps, where msl_set_beam has always queued them
        if ((rc = absorptive_transmission(h, 0, h->FB))) return rc;
        if (h->set.bl_on && (rc = bandlimit_lowpass(h, 0, h->FB))) return rc;
        if (h->tds_on && h->tds_W && (rc = tds_weights(h, false))) return rc;
        for (int f = 0; f < h->FB; ++f) if ((rc = transpose_odd_slices(h, f))) return rc;
    } else if ((rc = transmission_from_V(h, h->V, 0)) || (rc = finish_stacks(h, 0, 1))) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return MSL_OK;
}

// ---- invalidations ----
// The resident potential no longer counts (msl_propagate is MSL_ERR_STATE until the next build or upload)
void drop_potential(msl_handle* h) { h->have_potential = false; h->abs_built = false; h->ion_built = false; h->pg_valid = false; }

// A built S-matrix belongs to the tables and the stack it was built with: it has to be built again (the beams stay)
void drop_smatrix_result(msl_handle* h) { h->sm_built = false; }

// PRISM: free S, the beams and the coefficients (the stream is idle)
void smatrix_release(msl_handle* h) {
    h->sm_S.release(); h->sm_c.release(); h->sm_beams.release();
    h->sm_h.clear();
    h->sm_fx = h->sm_fy = h->sm_Bm = 0;
    h->sm_open = h->sm_built = false;
}

// TDS off: its buffers freed, and the handle back on the loop its tilt allows
int tds_clear(msl_handle* h) {
    if (!h->tds_on) return MSL_OK;
    h->tds_on = h->tds_have = false;
    h->tds_n = 0;
    h->tds_bits.release(); h->tds_g.release(); h->tds_W.release(); h->tds_acc.release(); h->tds_part.release();
    return set_loop_mode(h, allowed_onepass(h, h->set.tilt_tan[0], h->set.tilt_tan[1]));
}

// Ionisation off: its buffers freed, and the handle back on the loop its tilt allows
int ion_clear(msl_handle* h) {
    if (!h->ion_on) return MSL_OK;
    h->ion_on = h->ion_built = h->ion_have = false;
    h->ion_n = h->ion_nsp = 0;
    h->ion_tab.release(); h->ion_W.release(); h->ion_ones.release(); h->ion_part.release(); h->ion_acc.release(); h->ion_norm.release();
    return set_loop_mode(h, allowed_onepass(h, h->set.tilt_tan[0], h->set.tilt_tan[1]));
}

// The adjoint off: its buffers freed, and the handle back on the loop its tilt allows
int adj_clear(msl_handle* h) {
    if (!h->adj_on) return MSL_OK;
    h->adj_on = ADJ_OFF; h->adj_P = 0;
    h->adj_w.release(); h->adj_D.release(); h->adj_stack.release(); h->adj_grad.release(); h->adj_part.release(); h->adj_loss.release();
    h->pg_tiles.release(); h->pg_img.release(); h->pg_gamma.release(); h->pg_out.release();      // (the position chain's own: grown again on demand)
    return set_loop_mode(h, allowed_onepass(h, h->set.tilt_tan[0], h->set.tilt_tan[1]));
}

}  // namespace

// ---- the setters ----
extern "C" {

int msl_set_beam(msl_handle* h, double wavelength, double sigma, double dz) {
    if (!h) return fail(h, MSL_ERR_INVALID, "null handle");
    if (!(wavelength > 0)) return fail(h, MSL_ERR_INVALID, "msl_set_beam: wavelength must be positive");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (wavelength != h->cfg.wavelength) h->pm_valid = false;      // until the next msl_set_probes
    h->cfg.wavelength = wavelength; h->cfg.sigma = sigma; h->cfg.dz = dz;
    if (h->sm_open) {                                       // the wavelength changes the beam set
        HIPCHK(h, hipStreamSynchronize(h->stream));
        smatrix_release(h);
    }
    const int rc = refresh_propagator(h);                   // a tilt and a band limit stay on the handle
    if (rc || !h->have_potential) return rc;
    if (!h->abs_built && !h->V)
        return fail(h, MSL_ERR_STATE, "msl_set_beam: potential present but V not kept (keep_potential=0); rebuild the potential");
    return remake_transmission(h);
}

int msl_set_tilt(msl_handle* h, double tan_x, double tan_y) {
    if (!h) return fail(h, MSL_ERR_INVALID, "null handle");
    if (!std::isfinite(tan_x) || !std::isfinite(tan_y)) return fail(h, MSL_ERR_INVALID, "msl_set_tilt: tan_x and tan_y must be finite");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    int rc = set_loop_mode(h, allowed_onepass(h, tan_x, tan_y));      // the loop that can run this tilt; a refused switch leaves the handle as it was
    if (rc) return rc;
    const msl_handle::Settings old = h->set;
    h->set.tilt_tan[0] = tan_x; h->set.tilt_tan[1] = tan_y; h->set.tilt_set = true;
    if ((rc = refresh_propagator(h))) { h->set = old; return rc; }
    drop_smatrix_result(h);
    return MSL_OK;
}

int msl_get_tilt(const msl_handle* h, double* tan_xy) {
    if (!h || !tan_xy) return MSL_ERR_INVALID;
    tan_xy[0] = h->set.tilt_tan[0]; tan_xy[1] = h->set.tilt_tan[1];
    return MSL_OK;
}

int msl_set_bandlimit(msl_handle* h, int32_t cut_x, int32_t cut_y) {
    if (!h) return fail(h, MSL_ERR_INVALID, "null handle");
    const msl_config& c = h->cfg;
    const bool clear = cut_x < 0 && cut_y < 0;
    if (!clear) {
        if (cut_x < 1 || cut_y < 1)
            return fail(h, MSL_ERR_INVALID, "msl_set_bandlimit: cuts (%d, %d): both at least 1, or both negative to clear", cut_x, cut_y);
        if (3LL * cut_x >= c.nx || 3LL * cut_y >= c.ny)
            return fail(h, MSL_ERR_INVALID, "msl_set_bandlimit: cuts (%d, %d) are not alias-free on the %d x %d grid (3 cut < n)", cut_x, cut_y,
                        c.nx, c.ny);
    }
    if (clear && !h->set.bl_on) return MSL_OK;              // never set: the tables and the stacks stay what they are
    HIPCHK(h, hipSetDevice(c.device));
    int rc;
    if (!clear) {
        if ((rc = h->bl_mx.reserve(h, (size_t)c.nx)) || (rc = h->bl_my.reserve(h, (size_t)c.ny))) return rc;
        hipLaunchKernelGGL(bandlimit_mask_kernel, dim3((unsigned)((c.nx + BL_BLOCK - 1) / BL_BLOCK)), dim3(BL_BLOCK), 0, h->stream, c.nx, cut_x,
                           h->bl_mx.p);
        hipLaunchKernelGGL(bandlimit_mask_kernel, dim3((unsigned)((c.ny + BL_BLOCK - 1) / BL_BLOCK)), dim3(BL_BLOCK), 0, h->stream, c.ny, cut_y,
                           h->bl_my.p);
        HIPCHK(h, hipGetLastError());
    }
    const msl_handle::Settings old = h->set;
    h->set.bl_on = !clear;
    h->set.bl_cut[0] = clear ? -1 : cut_x; h->set.bl_cut[1] = clear ? -1 : cut_y;
    if ((rc = refresh_propagator(h))) { h->set = old; return rc; }
    drop_smatrix_result(h);
    // a kept V without absorption: the stack again from it under the new limit (what Propagate(..., bandlimit=) relies on).  Absorptive
    // stacks and a potential whose V was not kept belong to the limit they were built under: dropped, the next build makes them
    if (h->have_potential && h->V && !h->abs_built) return remake_transmission(h);
    drop_potential(h);
    return MSL_OK;
}

int msl_get_bandlimit(const msl_handle* h, int32_t* cut_xy) {
    if (!h || !cut_xy) return MSL_ERR_INVALID;
    cut_xy[0] = h->set.bl_cut[0]; cut_xy[1] = h->set.bl_cut[1];
    return MSL_OK;
}

// absorptive potential
int msl_set_absorption(msl_handle* h, const double* u_by_Z, int32_t absorb) {
    if (!h) return fail(h, MSL_ERR_INVALID, "msl_set_absorption: null handle");
    for (int z = 0; u_by_Z && z < 103; ++z)
        if (!std::isfinite(u_by_Z[z]) || !(u_by_Z[z] >= 0.0))
            return fail(h, MSL_ERR_INVALID, "msl_set_absorption: width %g of atomic number %d is not a finite number >= 0", u_by_Z[z], z + 1);
    if (u_by_Z && h->fin_R > 0)
        return fail(h, MSL_ERR_UNSUPPORTED, "msl_set_absorption: absorptive tables are not built under finite projection (msl_set_projection)");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipStreamSynchronize(h->stream));          // a queued build still reads the tables and the stacks
    h->ff_n = 0;                                         // d_ff holds f or f D: the next build makes its table again
    drop_potential(h);                                   // (Omega kept or left out, other widths: nothing msl_set_beam could remake t from)
    int rc;
    if ((!u_by_Z || !absorb) && (rc = tds_clear(h))) return rc;      // the TDS signal is that of the absorption: it goes with it
    if (!u_by_Z) {
        h->abs_on = h->abs_absorb = false;
        h->d_abs_u.release(); h->d_ffa.release(); h->abs_V.release(); h->abs_O.release();
        return MSL_OK;
    }
    if (!h->d_abs_u && (rc = h->d_abs_u.alloc(h, (size_t)103))) return rc;
    HIPCHK(h, hipMemcpy(h->d_abs_u, u_by_Z, 103 * sizeof(double), hipMemcpyHostToDevice));
    h->abs_on = true;
    h->abs_absorb = absorb != 0;
    return MSL_OK;
}

// TDS detector signal
int msl_set_tds(msl_handle* h, const uint16_t* member_bits, int32_t n_det) {
    if (!h) return fail(h, MSL_ERR_INVALID, "msl_set_tds: null handle");
    const bool clear = !member_bits || n_det == 0;
    if (!clear && (n_det < 1 || n_det > TDS_MAX)) return fail(h, MSL_ERR_INVALID, "msl_set_tds: %d detectors outside [1, %d]", n_det, TDS_MAX);
    if (!clear && !(h->abs_on && h->abs_absorb))
        return fail(h, MSL_ERR_STATE, "msl_set_tds: no absorption (call msl_set_absorption(.., absorb != 0) first)");
    if (!clear && h->FB > 1) return fail(h, MSL_ERR_UNSUPPORTED, "msl_set_tds: a frame batch of %d (the weight stack is that of one frame)", h->FB);
    if (!clear && h->ion_on) return fail(h, MSL_ERR_STATE, "msl_set_tds: msl_set_ionization is set (one per-slice reduction per handle)");
    if (!clear && h->adj_on) return fail(h, MSL_ERR_STATE, "msl_set_tds: msl_set_adjoint is set (its store takes the place of the reduction)");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipStreamSynchronize(h->stream));          // a queued build or loop still reads the tables and the stacks
    h->ff_n = 0;                                         // as msl_set_absorption: the next build makes the tables again
    drop_potential(h);
    int rc = tds_clear(h);
    if (rc || clear) return rc;
    const size_t npix = (size_t)h->cfg.nx * h->cfg.ny;
    if ((rc = h->tds_bits.alloc(h, npix))) return rc;
    HIPCHK(h, hipMemcpy(h->tds_bits, member_bits, npix * sizeof(uint16_t), hipMemcpyHostToDevice));
    h->tds_n = n_det;
    h->tds_on = true;
    rc = set_loop_mode(h, allowed_onepass(h, h->set.tilt_tan[0], h->set.tilt_tan[1]));
    if (rc) { h->tds_on = false; h->tds_n = 0; h->tds_bits.release(); }      // a refused switch: no TDS, as after the tds_clear above
    return rc;
}

// element maps
int msl_set_ionization(msl_handle* h, int32_t n, const int32_t* Z, const double* width, const double* cross_section) {
    if (!h) return fail(h, MSL_ERR_INVALID, "msl_set_ionization: null handle");
    const bool clear = n == 0 || !Z || !width || !cross_section;
    if (!clear && (n < 1 || n > ION_MAX)) return fail(h, MSL_ERR_INVALID, "msl_set_ionization: %d channels outside [1, %d]", n, ION_MAX);
    for (int e = 0; !clear && e < n; ++e) {
        if (Z[e] < 1 || Z[e] > 103) return fail(h, MSL_ERR_INVALID, "msl_set_ionization: atomic number %d of channel %d out of 1..103", Z[e], e);
        if (!std::isfinite(width[e]) || !(width[e] > 0.0))
            return fail(h, MSL_ERR_INVALID, "msl_set_ionization: width %g of channel %d is not a finite number > 0", width[e], e);
        if (!std::isfinite(cross_section[e]) || !(cross_section[e] >= 0.0))
            return fail(h, MSL_ERR_INVALID, "msl_set_ionization: cross-section %g of channel %d is not a finite number >= 0", cross_section[e], e);
    }
    if (clear && !h->ion_on) return MSL_OK;                 // never set: the handle stays what it is
    if (!clear && h->FB > 1)
        return fail(h, MSL_ERR_UNSUPPORTED, "msl_set_ionization: a frame batch of %d (the weight stack is that of one frame)", h->FB);
    if (!clear && h->tds_on) return fail(h, MSL_ERR_STATE, "msl_set_ionization: msl_set_tds is set (one per-slice reduction per handle)");
    if (!clear && h->adj_on) return fail(h, MSL_ERR_STATE, "msl_set_ionization: msl_set_adjoint is set (its store takes the place of the reduction)");
    if (!clear && h->fin_R > 0)
        return fail(h, MSL_ERR_UNSUPPORTED, "msl_set_ionization: the weight stack is not built under finite projection (msl_set_projection)");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipStreamSynchronize(h->stream));          // a queued build or loop still reads the tables and the stacks
    drop_potential(h);
    int rc = ion_clear(h);
    if (rc || clear) return rc;
    const size_t npix = (size_t)h->cfg.nx * h->cfg.ny;
    if ((rc = h->ion_ones.alloc(h, npix))) return rc;
    const float one = 1.0f;
    int one_bits;
    memcpy(&one_bits, &one, sizeof one_bits);
    HIPCHK(h, hipMemsetD32Async((hipDeviceptr_t)h->ion_ones.p, one_bits, npix, h->stream));
    for (int e = 0; e < n; ++e) { h->ion_Z[e] = Z[e]; h->ion_width[e] = width[e]; h->ion_cross[e] = cross_section[e]; }
    h->ion_n = n;
    h->ion_on = true;
    rc = set_loop_mode(h, allowed_onepass(h, h->set.tilt_tan[0], h->set.tilt_tan[1]));
    if (rc) { h->ion_on = false; h->ion_n = 0; h->ion_ones.release(); }     // a refused switch: no ionisation, as after the ion_clear above
    return rc;
}

// gradients
int msl_set_adjoint(msl_handle* h, int32_t loss_kind, double epsilon, const float* weight) {
    if (!h) return fail(h, MSL_ERR_INVALID, "msl_set_adjoint: null handle");
    const bool clear = loss_kind == ADJ_OFF;
    if (!clear && (loss_kind < ADJ_AMPLITUDE || loss_kind > ADJ_POISSON))
        return fail(h, MSL_ERR_INVALID, "msl_set_adjoint: loss %d outside [0, %d]", loss_kind, (int)ADJ_POISSON);
    // (the kernels hold epsilon in float32: one that rounds to zero there would divide by zero where |Psi| = 0)
    if (!clear && (!std::isfinite(epsilon) || !((float)epsilon > 0.f) || !std::isfinite((float)epsilon)))
        return fail(h, MSL_ERR_INVALID, "msl_set_adjoint: epsilon %g is not a finite float32 number > 0", epsilon);
    if (clear && !h->adj_on) return MSL_OK;                 // never set: the handle stays what it is
    const msl_config& c = h->cfg;
    if (!clear) {
        if (h->set.bl_on) return fail(h, MSL_ERR_UNSUPPORTED, "msl_set_adjoint: a band limit is set (its low-pass of t has no adjoint here)");
        if (h->abs_on) return fail(h, MSL_ERR_UNSUPPORTED, "msl_set_adjoint: an absorptive potential is set (t is not exp(i sigma V))");
        if (h->FB > 1) return fail(h, MSL_ERR_UNSUPPORTED, "msl_set_adjoint: a frame batch of %d (the wave stack is that of one frame)", h->FB);
        if (n_taps(h) > 0 || h->lr_on) return fail(h, MSL_ERR_UNSUPPORTED, "msl_set_adjoint: layers or a layer reduction are set");
        if (h->tds_on || h->ion_on) return fail(h, MSL_ERR_STATE, "msl_set_adjoint: a per-slice reduction is set (msl_set_tds / msl_set_ionization)");
    }
    HIPCHK(h, hipSetDevice(c.device));
    HIPCHK(h, hipStreamSynchronize(h->stream));          // a queued loop still reads the stacks
    int rc = adj_clear(h);
    if (rc || clear) return rc;
    const size_t npix = (size_t)c.nx * c.ny, P = (size_t)c.n_probes, slab = P * c.nx * h->pitch;
    const size_t want = (size_t)(c.nz - 1) * slab * sizeof(float2) + (size_t)c.nz * npix * sizeof(double) + P * npix * sizeof(float);
    if ((rc = h->adj_stack.alloc(h, (size_t)(c.nz - 1) * slab)) || (rc = h->adj_grad.alloc(h, (size_t)c.nz * npix)) ||
        (rc = h->adj_D.alloc(h, P * npix)) || (rc = h->adj_loss.alloc(h, P)) || (weight && (rc = h->adj_w.alloc(h, npix)))) {
        const std::string why = h->err;
        h->adj_on = ADJ_AMPLITUDE;                          // (so that adj_clear frees what was allocated)
        (void)adj_clear(h);
        return fail(h, rc, "msl_set_adjoint: the wave stack, the accumulator and the data of %d probes want %zu bytes (a smaller probe batch makes "
                           "the stack fit): %s", c.n_probes, want, why.c_str());
    }
    hipError_t e = weight ? hipMemcpy(h->adj_w, weight, npix * sizeof(float), hipMemcpyHostToDevice) : hipSuccess;
    if (e == hipSuccess) e = hipMemsetAsync(h->adj_grad, 0, (size_t)c.nz * npix * sizeof(double), h->stream);
    if (e != hipSuccess) {                                  // nothing stays allocated behind a failed set-up
        h->adj_on = ADJ_AMPLITUDE;
        (void)adj_clear(h);
        return fail(h, MSL_ERR_HIP, "msl_set_adjoint: the weight copy or the accumulator reset failed: %s", hipGetErrorString(e));
    }
    h->adj_eps = (float)epsilon;
    h->adj_P = c.n_probes;
    h->adj_on = loss_kind;
    rc = set_loop_mode(h, allowed_onepass(h, h->set.tilt_tan[0], h->set.tilt_tan[1]));
    if (rc) {                                               // a refused switch: no adjoint, as after the adj_clear above
        h->adj_on = ADJ_OFF; h->adj_P = 0;
        h->adj_w.release(); h->adj_D.release(); h->adj_stack.release(); h->adj_grad.release(); h->adj_loss.release();
    }
    return rc;
}

int msl_adjoint_reset(msl_handle* h) {
    if (!h) return fail(h, MSL_ERR_INVALID, "msl_adjoint_reset: null handle");
    if (!h->adj_on) return fail(h, MSL_ERR_STATE, "msl_adjoint_reset: no adjoint (msl_set_adjoint)");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipMemsetAsync(h->adj_grad, 0, h->adj_grad.n * sizeof(double), h->stream));
    return MSL_OK;
}

int msl_adjoint_add(msl_handle* h, const float* data, int32_t B, double* loss_out, void* probe_grad) {
    if (!h) return fail(h, MSL_ERR_INVALID, "msl_adjoint_add: null handle");
    if (!h->adj_on) return fail(h, MSL_ERR_STATE, "msl_adjoint_add: no adjoint (msl_set_adjoint)");
    if (!data || !loss_out) return fail(h, MSL_ERR_INVALID, "msl_adjoint_add: null argument");
    if (h->adj_P != h->cfg.n_probes)
        return fail(h, MSL_ERR_STATE, "msl_adjoint_add: the stack holds %d probes, the handle has %d (msl_set_adjoint after msl_resize_probes)", h->adj_P, h->cfg.n_probes);
    if (B < 1 || B > h->cfg.n_probes) return fail(h, MSL_ERR_INVALID, "msl_adjoint_add: %d probes, the handle has %d", B, h->cfg.n_probes);
    if (h->set.bl_on || h->abs_on || h->abs_built || n_taps(h) > 0 || h->lr_on)
        return fail(h, MSL_ERR_UNSUPPORTED, "msl_adjoint_add: a band limit, an absorptive potential or layers were set after msl_set_adjoint");
    if (!h->have_probes) return fail(h, MSL_ERR_STATE, "msl_adjoint_add: no probes (msl_set_probes / msl_upload_probes)");
    if (!h->have_potential) return fail(h, MSL_ERR_STATE, "msl_adjoint_add: no potential (msl_build_potential / msl_upload_potential)");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const int rc = adjoint_add(h, data, B, loss_out, (float2*)probe_grad);
    if (rc) (void)hipStreamSynchronize(h->stream);
    return rc;
}

int msl_adjoint_step_time(msl_handle* h, int32_t slice, int32_t reps, double* ms_step) {
    if (!h) return fail(h, MSL_ERR_INVALID, "msl_adjoint_step_time: null handle");
    if (!h->adj_on || h->adj_P != h->cfg.n_probes) return fail(h, MSL_ERR_STATE, "msl_adjoint_step_time: no adjoint (msl_set_adjoint)");
    if (!h->have_probes || !h->have_potential) return fail(h, MSL_ERR_STATE, "msl_adjoint_step_time: no probes or no potential");
    if (slice < 0 || slice >= h->cfg.nz) return fail(h, MSL_ERR_INVALID, "msl_adjoint_step_time: slice %d outside [0, %d)", slice, h->cfg.nz);
    if (reps < 1) return fail(h, MSL_ERR_INVALID, "msl_adjoint_step_time: reps must be positive");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    h->cur = nullptr;
    h->pm_g = 0;
    double ms = 0.0;
    EventPair timer;
    int rc = adjoint_step_launch(h, h->psi, slice, h->cfg.n_probes);            // one untimed launch first
    if (rc || (rc = timer.begin(h))) return rc;
    for (int r = 0; r < reps && rc == MSL_OK; ++r) rc = adjoint_step_launch(h, h->psi, slice, h->cfg.n_probes);
    if (rc || (rc = timer.end(h, &ms))) { (void)hipStreamSynchronize(h->stream); return rc; }
    if (ms_step) *ms_step = ms / reps;
    return MSL_OK;
}

int msl_adjoint_layout(const msl_handle* h, int32_t* pitch, int32_t* vec) {
    if (!h || !h->adj_on) return MSL_ERR_STATE;
    if (pitch) *pitch = h->pitch;
    if (vec) *vec = adjoint_step_vec(h, h->psi.p) ? 1 : 0;
    return MSL_OK;
}

int msl_adjoint_download(msl_handle* h, double* grad) {
    if (!h || !grad) return fail(h, MSL_ERR_INVALID, "msl_adjoint_download: null argument");
    if (!h->adj_on) return fail(h, MSL_ERR_STATE, "msl_adjoint_download: no adjoint (msl_set_adjoint)");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipMemcpyAsync(grad, h->adj_grad, h->adj_grad.n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return MSL_OK;
}

// gradients with respect to atom positions
int msl_adjoint_positions(msl_handle* h, const double* gamma, double* out) {
    if (!h || !out) return fail(h, MSL_ERR_INVALID, "msl_adjoint_positions: null argument");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const double* d_gamma = nullptr;
    int rc = position_prepare(h, "msl_adjoint_positions", gamma, &d_gamma);
    if (rc) return rc;
    h->cur = nullptr;
    std::vector<int> tile_of;
    int bins_used = 0, rows = 0;
    if ((rc = position_tiles(h, tile_of, bins_used, rows)) || (rc = position_chain(h, d_gamma, tile_of))) {
        (void)hipStreamSynchronize(h->stream);
        return rc;
    }
    const msl_config& c = h->cfg;
    const uint64_t npix = (uint64_t)c.nx * c.ny;
    // per slice the conversion and the transform (8 + 8 + 32 B per pixel); per bin with atoms one read of B_s and f_Z (12); per table
    // row its phases; the result
    h->ctr.algorithmic_bytes += (uint64_t)c.nz * npix * 48ull + (uint64_t)bins_used * npix * 12ull +
                                (uint64_t)rows * (uint64_t)(c.nx / 2 + 1 + c.ny / 2 + 1) * 8ull + (uint64_t)h->pg_n * 24ull;
    if (h->pg_n > 0)
        HIPCHK(h, hipMemcpyAsync(out, h->pg_out, (size_t)h->pg_n * 3 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return MSL_OK;
}

int64_t msl_adjoint_positions_rows(const msl_handle* h) {
    return (h && h->pg_valid && h->have_potential) ? h->pg_n : -1;
}

int msl_adjoint_positions_time(msl_handle* h, int32_t reps, double* ms_chain) {
    if (!h) return fail(h, MSL_ERR_INVALID, "msl_adjoint_positions_time: null handle");
    if (reps < 1) return fail(h, MSL_ERR_INVALID, "msl_adjoint_positions_time: reps must be positive");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const double* d_gamma = nullptr;
    int rc = position_prepare(h, "msl_adjoint_positions_time", nullptr, &d_gamma);
    if (rc) return rc;
    h->cur = nullptr;
    std::vector<int> tile_of;
    int bins_used = 0, rows = 0;
    double ms = 0.0;
    EventPair timer;
    if ((rc = position_tiles(h, tile_of, bins_used, rows)) || (rc = position_chain(h, d_gamma, tile_of)) || (rc = timer.begin(h))) {
        (void)hipStreamSynchronize(h->stream);
        return rc;
    }
    for (int r = 0; r < reps && rc == MSL_OK; ++r) rc = position_chain(h, d_gamma, tile_of);
    if (rc || (rc = timer.end(h, &ms))) { (void)hipStreamSynchronize(h->stream); return rc; }
    if (ms_chain) *ms_chain = ms / reps;
    return MSL_OK;
}

}  // extern "C"

namespace {

// ---- gradients with respect to scan positions and probe aberrations: the probe recipe backwards; adjoint.h ----
// the aperture's bounding box on one axis: signed frequencies |f| <= radius / kfreq (one more on either side against the rounding of
// the quotient -- the kernel's own test decides), cut to the axis' own range -(n / 2) .. (n - 1) / 2
void probe_box_axis(int n, double kfreq, double radius, int* lo, int* w) {
    const double q = radius / kfreq;
    const int reach = q < (double)n ? (int)q + 1 : n;
    const int a = std::max(-reach, -(n / 2)), b = std::min(reach, (n - 1) / 2);
    *lo = a; *w = b - a + 1;
}

struct ProbeChain {
    ProbeBox box;
    long long tiles;
};

int probe_params_prepare(msl_handle* h, const char* who, int B, ProbeChain* pc) {
    if (B < 1 || B > h->cfg.n_probes) return fail(h, MSL_ERR_INVALID, "%s: %d probes, the handle has %d", who, B, h->cfg.n_probes);
    if (!h->pm_valid || !h->have_probes)
        return fail(h, MSL_ERR_STATE, "%s: the probe buffer does not hold probes of msl_set_probes at a convergent aperture (mrad > 0) with the "
                                      "aberrations and the wavelength of today: call msl_set_probes (msl_upload_probes, msl_shift_probes, "
                                      "msl_set_probe_members, the PRISM calls, msl_resize_probes, msl_set_aberrations and a changed wavelength "
                                      "drop the recipe this call differentiates)", who);
    const msl_config& c = h->cfg;
    const double radius = (h->pm_mrad * 1e-3) / h->pm_wavelength;
    probe_box_axis(c.nx, 1.0 / (c.nx * c.dx), radius, &pc->box.x_lo, &pc->box.wx);
    probe_box_axis(c.ny, 1.0 / (c.ny * c.dy), radius, &pc->box.y_lo, &pc->box.wy);
    pc->tiles = ((long long)pc->box.wx * pc->box.wy + PM_TILE - 1) / PM_TILE;
    if (pc->tiles > 0x7fffffffLL) return fail(h, MSL_ERR_UNSUPPORTED, "%s: too many tiles", who);
    if (B > 65535) return fail(h, MSL_ERR_UNSUPPORTED, "%s: %d probes in one call, the grid takes 65535", who, B);
    int rc;
    if ((rc = h->pm_part.reserve(h, (size_t)pc->tiles * c.n_probes * PM_SLOTS)) || (rc = h->pm_sums.reserve(h, (size_t)c.n_probes * PM_SLOTS)))
        return rc;
    return MSL_OK;
}

// the work buffer's first B images -> their transforms in place, then pm_sums (B, PM_SLOTS): queued
int probe_params_chain(msl_handle* h, int B, const ProbeChain& pc) {
    const msl_config& c = h->cfg;
    int rc;
    if ((rc = fft2_inplace(h, h->psi, B, +1, 1.0f, h->pitch))) return rc;
    hipLaunchKernelGGL(probe_moment_kernel, dim3((unsigned)pc.tiles, (unsigned)B), dim3(256), 0, h->stream, (const float2*)h->psi.p,
                       (const double*)h->pm_dxy.p, B, c.nx, c.ny, h->pitch, pc.box, 1.0 / (c.nx * c.dx), 1.0 / (c.ny * c.dy), 1.0 / (c.nx * c.dx),
                       1.0 / (c.ny * c.dy), (h->pm_mrad * 1e-3) / h->pm_wavelength, h->pm_wavelength, h->pm_ab, h->pm_part.p);
    hipLaunchKernelGGL((slice_sums_finish_kernel<double, PM_SLOTS>), dim3((unsigned)((B * PM_SLOTS + 255) / 256)), dim3(256), 0, h->stream,
                       (const double*)h->pm_part.p, pc.tiles, B, PM_SLOTS, h->pm_sums.p);
    HIPCHK(h, hipGetLastError());
    return mark_launch(h, K_OTHER);
}

}  // namespace

extern "C" {

int msl_adjoint_probe_params(msl_handle* h, const void* g0, int32_t B, double* out) {
    if (!h || !out) return fail(h, MSL_ERR_INVALID, "msl_adjoint_probe_params: null argument");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const msl_config& c = h->cfg;
    ProbeChain pc;
    int rc = probe_params_prepare(h, "msl_adjoint_probe_params", B, &pc);
    if (rc) return rc;
    if (!g0 && (h->pm_g < B || h->have_exit))
        return fail(h, MSL_ERR_STATE, "msl_adjoint_probe_params: g0 == NULL needs the probe gradient of %d images that msl_adjoint_add leaves in the "
                                      "work buffer (it holds %d)", B, h->have_exit ? 0 : h->pm_g);
    h->cur = nullptr;
    h->pm_g = 0; h->have_exit = false;                      // the work buffer ends as the transforms
    if (g0)
        HIPCHK(h, hipMemcpy2DAsync(h->psi, (size_t)h->pitch * sizeof(float2), g0, (size_t)c.ny * sizeof(float2), (size_t)c.ny * sizeof(float2),
                                   (size_t)B * c.nx, hipMemcpyHostToDevice, h->stream));
    if ((rc = probe_params_chain(h, B, pc))) { (void)hipStreamSynchronize(h->stream); return rc; }
    std::vector<double> sums((size_t)B * PM_SLOTS);
    HIPCHK(h, hipMemcpyAsync(sums.data(), h->pm_sums, sums.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    // per image the transform (32 B per pixel), the box's read of it, the partial rows and their sum
    h->ctr.algorithmic_bytes += (uint64_t)B * ((uint64_t)c.nx * c.ny * 32ull + (uint64_t)pc.box.wx * pc.box.wy * 8ull + (uint64_t)pc.tiles * PM_SLOTS * 16ull);
    const double f = 4.0 * M_PI / ((double)c.nx * c.ny);
    for (int p = 0; p < B; ++p) {
        const double* s = sums.data() + (size_t)p * PM_SLOTS;
        double* o = out + (size_t)p * 30;
        o[0] = -f * s[0]; o[1] = -f * s[1];
        for (int j = 0; j < 14; ++j) { o[2 + 2 * j] = f * s[2 + j]; o[3 + 2 * j] = 0.0; }
        for (int k = 0; k < 11; ++k) o[3 + 2 * PM_B_TERM[k]] = f * s[16 + k];
    }
    return MSL_OK;
}

int msl_adjoint_probe_params_time(msl_handle* h, int32_t reps, double* ms_chain) {
    if (!h) return fail(h, MSL_ERR_INVALID, "msl_adjoint_probe_params_time: null handle");
    if (reps < 1) return fail(h, MSL_ERR_INVALID, "msl_adjoint_probe_params_time: reps must be positive");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    ProbeChain pc;
    const int B = h->cfg.n_probes;
    int rc = probe_params_prepare(h, "msl_adjoint_probe_params_time", B, &pc);
    if (rc) return rc;
    h->cur = nullptr;
    h->pm_g = 0; h->have_exit = false;
    double ms = 0.0;
    EventPair timer;
    if ((rc = probe_params_chain(h, B, pc)) || (rc = timer.begin(h))) { (void)hipStreamSynchronize(h->stream); return rc; }
    for (int r = 0; r < reps && rc == MSL_OK; ++r) rc = probe_params_chain(h, B, pc);
    if (rc || (rc = timer.end(h, &ms))) { (void)hipStreamSynchronize(h->stream); return rc; }
    if (ms_chain) *ms_chain = ms / reps;
    return MSL_OK;
}

}  // extern "C"

namespace {

// Projected potentials + transmission functions of `count` MD frames (the same atoms, `count` sets of positions) into the batch
// slots first_slot .. first_slot + count - 1: ONE launch each of the atom preparation, the stable counting sort (keys = frame x
// slice x species), the two phase tables, the structure factor and the two inverse-transform passes for as many frames as the
// phase tables of a group may take (6 GB), instead of that sequence per frame.  The reference builds one Potential per frame
// (calculators.py:172-186, potentials.py:188-348); with its default single probe that build IS the frame (round 2: 0.43 of
// 0.62 ms at 512^2 x 100 slices, of which ~110 us were launches of 5-15 us kernels and four small copies per frame).
// With `th` the frames are generated from the resident structure (msl_build_thermal, msl_build_modes): pos and Z are not read, the
// species maps are the ones msl_set_structure made, and stage_thermal or stage_modes takes the place of stage_atoms; everything
// behind d_pos is the same.
int build_potentials(msl_handle* h, const double* pos, const int32_t* Z, int64_t n, int count, int first_slot, int32_t ax1, int32_t ax2, int32_t axs,
                     const GeneratedSource* th = nullptr) {
    const msl_config& c = h->cfg;
    const size_t npix = (size_t)c.nx * c.ny;
    PotGroup p{};
    int rc = MSL_OK;
    h->pg_valid = false;                                 // the tables are rewritten: msl_adjoint_positions needs this build to finish
    if (th) {
        memcpy(p.z2s, h->th_map_z2s, sizeof p.z2s);
        memcpy(p.species, h->th_map_species, sizeof p.species);
        p.nsp = h->th_nsp;
    } else {
        rc = map_species(h, Z, n, p);
    }
    if (rc) return rc;
    // with launch timing off the call only queues work: no event, no host wait (the frames of a run pipeline on the stream)
    EventPair timer;
    if (c.launch_timing && (rc = timer.begin(h))) return rc;
    // finite projection: every atom is rep weighted rows, every species (2 R + 1) J channel tables
    p.finite = h->fin_R > 0;
    p.rep = p.finite ? 2 * (2 * h->fin_R + 1) : 1;
    p.ntab = p.finite ? p.nsp * (2 * h->fin_R + 1) * h->fin_J : p.nsp;
    if (p.finite) {
        if (h->abs_on) return fail(h, MSL_ERR_UNSUPPORTED, "finite projection: absorptive or TDS tables are not built with it");
        if ((int)h->h_lo.size() != c.nz) return fail(h, MSL_ERR_STATE, "finite projection: msl_set_slices has not been called");
        for (int s = 1; s + 1 < c.nz; ++s)
            if (!(std::fabs((h->h_hi[s] - h->h_lo[s]) - c.dz) <= 1e-9 * std::fabs(c.dz)))
                return fail(h, MSL_ERR_UNSUPPORTED, "finite projection: slice %d is %.12g thick, the handle's dz is %.12g (uniform slices only)",
                            s, h->h_hi[s] - h->h_lo[s], c.dz);
        if (!(c.dz > 0)) return fail(h, MSL_ERR_UNSUPPORTED, "finite projection: dz must be positive");
        if ((long long)n * p.rep > 0x7fffffffLL || (long long)c.nz * p.ntab * std::max(1, count) > 0x7fffffffLL)
            return fail(h, MSL_ERR_UNSUPPORTED, "finite projection: %lld rows per frame or %lld bins exceed 2^31", (long long)n * p.rep,
                        (long long)c.nz * p.ntab * count);
    }
    if (p.ntab > h->ff_species_cap) {
        if ((rc = h->d_ff.alloc(h, npix * p.ntab))) return rc;
        h->ff_species_cap = p.ntab;
        h->ff_n = 0;
    }
    p.n = n; p.ax1 = ax1; p.ax2 = ax2; p.axs = axs;
    p.cx = c.nx / 2 + 1; p.cy = c.ny / 2 + 1; p.keys_per_frame = c.nz * std::max(p.ntab, 1);
    p.half_rows = pot_half_rows(h);
    if (h->abs_on) {
        // the absorptive build inverse-transforms with ifft_inplace's passes whatever pot_ifft is: half rows where those mirror them
        p.half_rows = h->Rx && h->Ry;
        const size_t stacks = npix * c.nz * h->FB;
        if (!h->abs_V) {
            if ((rc = h->abs_V.alloc(h, stacks))) return rc;
            HIPCHK(h, hipMemsetAsync(h->abs_V, 0, stacks * sizeof(float), h->stream));
        }
        if (h->abs_absorb && !h->abs_O) {
            if ((rc = h->abs_O.alloc(h, stacks))) return rc;
            HIPCHK(h, hipMemsetAsync(h->abs_O, 0, stacks * sizeof(float), h->stream));
        }
    }
    const size_t frame_rows = (size_t)n * p.rep;            // rows of the sort and of the phase tables per frame
    p.sf_stream = (double)frame_rows / std::max(1, p.keys_per_frame) >= 128.0 && !dbg_env("MSL_SF_TILED");
    p.vscale = (float)(1.0 / ((double)c.nx * c.ny) / (c.dx * c.dx * c.dy * c.dy));
    // frames per group: the phase tables of a group (n atoms x (nx/2 + 1 + ny/2 + 1) x 8 bytes per frame) stay under 6 GB
    const size_t table_bytes_per_frame = std::max<size_t>(1, frame_rows * (size_t)(p.cx + p.cy) * sizeof(float2));
    const int G = (int)std::max<size_t>(1, std::min<size_t>((size_t)count, (size_t)6e9 / table_bytes_per_frame));
    const int nkeys_cap = p.keys_per_frame * G;
    if (nkeys_cap > h->keys_cap) {
        if ((rc = h->d_counts.alloc(h, (size_t)nkeys_cap + 1)) || (rc = h->d_start.alloc(h, (size_t)nkeys_cap + 1))) return rc;
        h->keys_cap = nkeys_cap;
    }
    if ((rc = ensure_atoms(h, frame_rows * G, frame_rows * G + (size_t)(SF_ALIGN - 1) * nkeys_cap))) return rc;
    for (int f0 = 0; f0 < count; f0 += G) {
        p.g = std::min(G, count - f0); p.slot = first_slot + f0;
        p.TR = h->trans + (size_t)p.slot * c.nz * npix;
        p.TRT = h->transT ? h->transT + (size_t)p.slot * c.nz * npix : nullptr;
        p.n_slices = c.nz * p.g; p.nkeys = p.keys_per_frame * p.g;
        p.rows = (long long)frame_rows * p.g; p.rows_pad = p.rows + (long long)(SF_ALIGN - 1) * p.nkeys;
        if (n > 0 && p.nsp > 0) {
            rc = !th ? stage_atoms(h, p, pos + (size_t)f0 * n * 3, Z, f0 == 0)
                 : th->modes ? stage_modes(h, p, th->seed, th->first + (uint64_t)f0, f0 == 0)
                             : stage_thermal(h, p, th->seed, th->first + (uint64_t)f0, f0 == 0);
            if (rc || (rc = bin_atoms(h, p)) || (h->ion_on && (rc = ionization_group(h, p, true))) ||
                (!h->abs_on && (rc = launch_structure_factor(h, p)))) return rc;
        } else {
            if (h->ion_on && (rc = ionization_group(h, p, false))) return rc;
            if (!h->abs_on) HIPCHK(h, hipMemsetAsync(p.TR, 0, npix * p.n_slices * sizeof(float2), h->stream));
        }
        if ((rc = h->abs_on ? absorptive_group(h, p, n > 0 && p.nsp > 0) : potential_ifft(h, p))) return rc;
    }
    h->n_species = p.nsp;
    h->fin_nch = p.finite ? p.ntab : 0;
    if (h->set.bl_on && (rc = bandlimit_built(h, first_slot, count))) return rc;
    if ((rc = timer.end(h, &h->ctr.ms_potential))) return rc;
    h->have_potential = true;
    h->abs_built = h->abs_on;
    h->ion_built = h->ion_on;
    // the tables of one frame of the caller's atoms, plain projection: what msl_adjoint_positions differentiates
    // (a band limit low-passes V behind the structure factor: the chain would differentiate the unfiltered build)
    h->pg_valid = !th && count == 1 && !p.finite && !h->abs_on && !h->set.bl_on;
    h->pg_n = n; h->pg_nsp = p.nsp; h->pg_ax1 = ax1; h->pg_ax2 = ax2;
    return MSL_OK;
}

}  // namespace

// ---- TACAW time transform -----------------------------------------------------
// The kernel that transforms T frames of images of npix pixels along time (plan_time), in the order of precedence:
//   TK_FOURSTEP  1024 frames of images beyond the wave-split kernel's 32-bit offsets: the four-step column kernel, R = 32 (it served
//                256 and 1024 frames until the split kernel overtook it: T = 256, 64 probes x 1024^2 40.2 -> 39.7 ms, 16 x 2048^2
//                44.7 -> 40.7 ms; T = 1024, 8 x 1024^2 33.7 -> 29.3 ms)
//   TK_DIRECT    smooth counts from 16 to 128 (100 = 4.5.5 ...): a lane per pixel, the whole time line in its registers (time_direct_kernel)
//   TK_SPLIT     smooth counts up to 1024: the register network split over the waves of a workgroup (time_split_kernel; tsplit_tw)
//   TK_CHIRPZ    any other count up to 512: chirp-z on the register FFTs (time_cz_kernel; the tables `opt`)
//   TK_GENERIC   the generic LDS kernel (plan_t)
// The per-lane / wave-split kernels (70 instantiations) are compiled in translation units of their own (tacaw_direct.hip,
// tacaw_split.hip, tacaw_split2.hip: built in parallel with this file); tacaw_launch.h declares their launchers.
enum TimeKind { TK_FOURSTEP, TK_DIRECT, TK_SPLIT, TK_CHIRPZ, TK_GENERIC };

static TimeKind plan_time(const msl_handle* h, int T, int64_t npix) {
    if (h->cfg.fft_path != 0 || dbg_env("MSL_TACAW_GENERIC")) return TK_GENERIC;
    const bool regs = !dbg_env("MSL_TACAW_CHIRPZ");                  // the per-lane and the wave-split register kernels
    // 32-bit offsets: the buffer unit adds the lane offset and the scalar row offset in 32 bits (measured: the sum wraps) --
    // pixel + up to 64 rows with one block per wave, pixel + TP + (TP + 1) / 2 rows with two; time_split_launch falls back from the
    // two-block shape to the one-block shape of the same L where there is one (L = 2, 4: up to 512 frames)
    const bool split = regs && time_split_fits(T, npix) && !(T == 1024 && dbg_env("MSL_TACAW_FOURSTEP"));
    if (T == 1024 && !split && npix % 16 == 0 && npix >= 32) return TK_FOURSTEP;
    if (regs && time_direct_has(T) && (unsigned long long)((T + 1) / 2) * (unsigned long long)npix * 8ull < (1ull << 32)) return TK_DIRECT;
    if (split) return TK_SPLIT;
    return T <= 512 ? TK_CHIRPZ : TK_GENERIC;
}

// W_T^n, n < T, for the cross-wave butterflies of time_split_kernel (the cache is invalid while it is rebuilt)
static int make_tsplit_table(msl_handle* h, int T) {
    if (h->tsplit_T == T) return MSL_OK;
    h->tsplit_T = 0;
    std::vector<float2> w(T);
    for (int n = 0; n < T; ++n) { const double a = -2.0 * M_PI * (double)n / (double)T; w[n] = make_float2((float)cos(a), (float)sin(a)); }
    int rc = h->tsplit_tw.alloc(h, (size_t)T);
    if (rc) return rc;
    HIPCHK(h, hipMemcpy(h->tsplit_tw, w.data(), (size_t)T * sizeof(float2), hipMemcpyHostToDevice));
    h->tsplit_T = T;
    return MSL_OK;
}

static int launch_time_cz(msl_handle* h, const TimeJob& j) {
    const int T = j.T;
    const long long npix = j.npix, batch = j.n_images;
    auto launch = [&](auto r_c, auto cols_c, auto vec_c) -> int {
        constexpr int R = decltype(r_c)::value, COLS = decltype(cols_c)::value;
        constexpr bool VEC = decltype(vec_c)::value;
        constexpr int M = R * R, NH = M / 2;
        const size_t lds = ((size_t)M + NH + 2 + NH + (size_t)2 * COLS * tcz_stride(R, T)) * 8;          // two tile buffers
        const long long tiles = ((npix + COLS - 1) / COLS) * batch;
        const int per_cu = std::max(1, std::min(2, (int)((size_t)h->lds_limit / lds)));
        const int grid = (int)std::min<long long>(tiles, (long long)h->n_cus * per_cu);
        return launch_lds(h, time_cz_kernel<R, COLS, VEC>, dim3(grid), dim3(COLS * R), lds, K_OTHER, j);
    };
    using I16 = std::integral_constant<int, 16>; using I32 = std::integral_constant<int, 32>;
    const bool even = (npix % 2 == 0);
    if (h->opt.R == 16) return even ? launch(I16{}, I32{}, std::true_type{}) : launch(I16{}, I32{}, std::false_type{});
    return even ? launch(I32{}, I16{}, std::true_type{}) : launch(I32{}, I16{}, std::false_type{});
}

// |FFT_t|^2 of `batch` (T, npix) blocks of complex spectra src -> dst (float32), DC removed and fftshifted (msl_tacaw)
static int tacaw_run(msl_handle* h, const float2* src, float* dst, int64_t batch, int32_t T, int64_t npix) {
    if (T < 2) return fail(h, MSL_ERR_INVALID, "msl_tacaw: needs at least 2 frames (got %d)", T);
    if (batch < 1 || npix < 1) return fail(h, MSL_ERR_INVALID, "msl_tacaw: bad batch/npix");
    if (npix > 0x7fffffffLL) return fail(h, MSL_ERR_UNSUPPORTED, "msl_tacaw: npix too large");
    const TimeKind kind = plan_time(h, T, npix);
    int rc = MSL_OK;
    DevBuf<float2> tw4_t;
    switch (kind) {
    case TK_FOURSTEP: rc = make_tw4(h, tw4_t, 32); break;
    case TK_DIRECT:   break;
    case TK_SPLIT:    rc = make_tsplit_table(h, T); break;
    case TK_CHIRPZ:
        if (h->opt_T != T) {
            h->opt_T = 0;
            if ((rc = make_cz_tables(h, h->opt, T))) return rc;                   // (M = 256 below 33 frames as well)
            h->opt_T = T;
        }
        break;
    case TK_GENERIC:  rc = make_plan(h, h->plan_t, T); break;
    }
    if (rc) return rc;
    TimeJob j{};
    j.in = src; j.out = dst;
    j.image_stride = (long long)T * npix; j.npix = (int)npix; j.n_images = (int)batch; j.T = T;
    EventPair timer;
    if ((rc = timer.begin(h))) return rc;
    h->cur = nullptr;
    switch (kind) {
    case TK_FOURSTEP: {
        // time lines are "columns" of a (T, npix) image per probe: 16 neighbouring pixels per tile
        ColJob c{};
        c.in = src; c.out = nullptr; c.px = nullptr; c.tw = tw4_t; c.out_real = dst;
        c.in_image_stride = c.out_image_stride = j.image_stride;
        c.in_pitch = c.out_pitch = (int)npix; c.ny = (int)npix; c.n_images = (int)batch;
        c.flags = COL_FWD | COL_INTENSITY; c.scale = 1.f;
        rc = launch_col_fast_r<32>(h, c, K_OTHER);
        break;
    }
    case TK_DIRECT:
        if (!time_direct_launch(j, h->n_cus, h->stream)) return fail(h, MSL_ERR_UNSUPPORTED, "no per-lane time kernel for %d frames", T);
        HIPCHK(h, hipGetLastError());
        rc = mark_launch(h, K_OTHER);
        break;
    case TK_SPLIT:
        j.tw = h->tsplit_tw;
        if (!time_split_launch(j, h->n_cus, (size_t)h->lds_limit, h->stream)) return fail(h, MSL_ERR_UNSUPPORTED, "no wave-split time kernel for %d frames", T);
        HIPCHK(h, hipGetLastError());
        rc = mark_launch(h, K_OTHER);
        break;
    case TK_CHIRPZ:
        j.tw = h->opt.tw; j.bf = h->opt.bf; j.bw = h->opt.bw;
        rc = launch_time_cz(h, j);
        break;
    case TK_GENERIC: {
        LineArgs a;
        a.in = src; a.out = nullptr; a.out_real = dst;
        a.n_lines = (long long)batch * npix; a.lines_per_image = (int)npix;
        a.in_es = a.out_es = npix; a.in_ls = a.out_ls = 1; a.in_is = a.out_is = j.image_stride;
        a.contiguous_lines = 1; a.fft1 = +1; a.store_mode = STORE_INTENSITY; a.shift_n = T / 2;
        rc = launch_lines(h, h->plan_t, a, K_OTHER);
        break;
    }
    }
    return rc ? rc : timer.end(h, &h->ctr.ms_tacaw);
}

// msl_tacaw on one (P, T, wpitch) block of the resident result, into the handle's intensity buffer
static int tacaw_resident(msl_handle* h, const float2* block) {
    const msl_config& c = h->cfg;
    // the pad pixels of an image are pixels like any other here (zeros in, zeros out)
    const size_t need = (size_t)c.n_probes * c.n_frames * h->wpitch;
    int rc;
    if (h->intensity.n != need && (rc = h->intensity.alloc(h, need))) return rc;
    h->intensity_F = c.n_frames; h->intensity_ld = h->wpitch;
    return tacaw_run(h, block, h->intensity, c.n_probes, c.n_frames, (int64_t)h->wpitch);
}

// ---- windowed, segment-averaged spectra (tacaw_welch.h) ----
// the checks of msl_tacaw_welch that need no device, and g = w sqrt(L / (S sum w^2)) in float64 -> float32
static int welch_table(msl_handle* h, int32_t T, int32_t L, int32_t hop, const double* window, int* S_out, std::vector<float>& g) {
    if (T < 2) return fail(h, MSL_ERR_INVALID, "msl_tacaw_welch: needs at least 2 frames (got %d)", T);
    if (L > T) return fail(h, MSL_ERR_INVALID, "msl_tacaw_welch: segment length %d exceeds the %d frames", L, T);
    if (L < 1 || hop < 1 || hop > L) return fail(h, MSL_ERR_INVALID, "msl_tacaw_welch: hop %d outside [1, %d]", hop, L);
    double sw2 = 0.0;
    for (int n = 0; n < L; ++n) {
        const double w = window ? window[n] : 1.0;
        if (!(w >= 0.0) || !std::isfinite(w)) return fail(h, MSL_ERR_INVALID, "msl_tacaw_welch: window[%d] = %g is negative or not finite", n, w);
        sw2 += w * w;
    }
    if (!(sw2 > 0.0)) return fail(h, MSL_ERR_INVALID, "msl_tacaw_welch: the window is zero everywhere");
    if (!time_welch_has(L)) return fail(h, MSL_ERR_UNSUPPORTED, "msl_tacaw_welch: no kernel for segment length %d (2-3-5-7-smooth lengths 16 ... 128)", L);
    const int S = 1 + (T - L) / hop;
    const double norm = std::sqrt((double)L / ((double)S * sw2));
    g.resize(L);
    for (int n = 0; n < L; ++n) g[n] = (float)((window ? window[n] : 1.0) * norm);
    *S_out = S;
    return MSL_OK;
}

// `batch` (T, npix) blocks of complex spectra src -> (L, npix) blocks of float32 Welch intensities dst (msl_tacaw_welch)
static int welch_run(msl_handle* h, const float2* src, float* dst, int64_t batch, int32_t T, int64_t npix, int32_t L, int32_t hop, int S,
                     const std::vector<float>& g) {
    if (batch < 1 || npix < 1) return fail(h, MSL_ERR_INVALID, "msl_tacaw_welch: bad batch/npix");
    if (npix > 0x7fffffffLL || batch > 0x7fffffffLL) return fail(h, MSL_ERR_UNSUPPORTED, "msl_tacaw_welch: npix or batch too large");
    // 32-bit offsets, as for time_direct_kernel: the lane's pixel plus up to (L + 1) / 2 rows through one descriptor
    if ((unsigned long long)((L + 1) / 2) * (unsigned long long)npix * 8ull >= (1ull << 32))
        return fail(h, MSL_ERR_UNSUPPORTED, "msl_tacaw_welch: images of %lld pixels leave the 32-bit row offsets at segment length %d", (long long)npix, L);
    int rc;
    if (h->welch_g_host != g || !h->welch_g) {
        // (an earlier launch on the stream may still read the old table)
        HIPCHK(h, hipStreamSynchronize(h->stream));
        h->welch_g_host.clear();
        if ((rc = h->welch_g.reserve(h, (size_t)TDIR_MAX))) return rc;
        HIPCHK(h, hipMemcpy(h->welch_g, g.data(), (size_t)L * sizeof(float), hipMemcpyHostToDevice));
        h->welch_g_host = g;
    }
    WelchJob j{};
    j.in = src; j.out = dst; j.g = h->welch_g;
    j.in_image_stride = (long long)T * npix; j.out_image_stride = (long long)L * npix;
    j.npix = (int)npix; j.n_images = (int)batch; j.L = L; j.hop = hop; j.S = S;
    EventPair timer;
    if ((rc = timer.begin(h))) return rc;
    h->cur = nullptr;
    if (!time_welch_launch(j, h->n_cus, h->stream)) return fail(h, MSL_ERR_UNSUPPORTED, "msl_tacaw_welch: no kernel for segment length %d", L);
    HIPCHK(h, hipGetLastError());
    if ((rc = mark_launch(h, K_OTHER))) return rc;
    h->ctr.algorithmic_bytes += (uint64_t)batch * (uint64_t)npix * (8ull * (uint64_t)S * (uint64_t)L + 4ull * (uint64_t)L);
    return timer.end(h, &h->ctr.ms_tacaw);
}

// msl_tacaw_welch on one (P, T, wpitch) block of the resident result, into the handle's intensity buffer: (P, L, wpitch)
static int welch_resident(msl_handle* h, const float2* block, int32_t L, int32_t hop, const double* window) {
    const msl_config& c = h->cfg;
    int S = 0, rc;
    std::vector<float> g;
    if ((rc = welch_table(h, c.n_frames, L, hop, window, &S, g))) return rc;
    const size_t need = (size_t)c.n_probes * L * h->wpitch;
    if (h->intensity.n != need && (rc = h->intensity.alloc(h, need))) return rc;
    h->intensity_F = L; h->intensity_ld = h->wpitch;
    return welch_run(h, block, h->intensity, c.n_probes, c.n_frames, (int64_t)h->wpitch, L, hop, S, g);
}

// The work buffers sized by the probe count (FB frames of n_probes images each; pitch, pitchT, onepass and need_psi0T are set)
static int alloc_probe_buffers(msl_handle* h, int n_probes) {
    const msl_config& c = h->cfg;
    const size_t images = (size_t)n_probes * h->FB, elems = (size_t)c.nx * h->pitch * images, elemsT = (size_t)c.ny * h->pitchT * images;
    int rc;
    if ((rc = h->psi0.alloc(h, elems)) || (rc = h->psi.alloc(h, elems))) return rc;
    if (h->onepass_planned && ((rc = h->psiT.alloc(h, elemsT)) || (h->need_psi0T && (rc = h->psi0T.alloc(h, elemsT))))) return rc;
    return h->d_xy.alloc(h, (size_t)2 * n_probes);
}

extern "C" {

int msl_abi_version(void) { return MSL_ABI_VERSION; }

int msl_line_kernel_class(int32_t n) {
    if (n == 256 || n == 512 || n == 1024 || n == 2048) return 2;
    int A = 0, B = 0, G = 0;
    return rowTM_factors(n, &A, &B, &G) ? 1 : 0;
}

const char* msl_last_error(const msl_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int msl_create(const msl_config* cfg, msl_handle** out) {
    if (!cfg || !out) return fail(nullptr, MSL_ERR_INVALID, "msl_create: null argument");
    *out = nullptr;
    if (cfg->nx < 2 || cfg->ny < 2 || cfg->nz < 1 || cfg->n_probes < 1 || cfg->n_frames < 0)
        return fail(nullptr, MSL_ERR_INVALID, "msl_create: bad grid nx=%d ny=%d nz=%d P=%d T=%d", cfg->nx, cfg->ny, cfg->nz,
                    cfg->n_probes, cfg->n_frames);
    if (!(cfg->dx > 0) || !(cfg->dy > 0) || !(cfg->wavelength > 0))
        return fail(nullptr, MSL_ERR_INVALID, "msl_create: dx, dy, wavelength must be positive");
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0)
        return fail(nullptr, MSL_ERR_HIP, "msl_create: no HIP device available (%s)", hipGetErrorString(e));
    if (cfg->device < 0 || cfg->device >= ndev)
        return fail(nullptr, MSL_ERR_INVALID, "msl_create: device %d out of range (have %d)", cfg->device, ndev);
    if (cfg->window_nx < 0 || cfg->window_nx > cfg->nx || cfg->window_ny < 0 || cfg->window_ny > cfg->ny)
        return fail(nullptr, MSL_ERR_INVALID, "msl_create: k-window %d x %d outside the %d x %d grid", cfg->window_nx, cfg->window_ny,
                    cfg->nx, cfg->ny);
    msl_handle* h = new (std::nothrow) msl_handle();
    if (!h) return fail(nullptr, MSL_ERR_NOMEM, "msl_create: out of host memory");
    h->cfg = *cfg;
    h->FB = (cfg->frame_batch > 1 && !cfg->keep_potential) ? cfg->frame_batch : 1;
    // k-window, centred on the DC pixel of the fftshifted spectrum (index n/2): [n/2 - w/2, n/2 - w/2 + w)
    h->wx = cfg->window_nx ? cfg->window_nx : cfg->nx;
    h->wy = cfg->window_ny ? cfg->window_ny : cfg->ny;
    h->wx0 = cfg->nx / 2 - h->wx / 2;
    h->wy0 = cfg->ny / 2 - h->wy / 2;
    h->bx = cfg->bin_nx > 1 ? cfg->bin_nx : 1;
    h->by = cfg->bin_ny > 1 ? cfg->bin_ny : 1;
    if (h->wx % h->bx || h->wy % h->by) {
        const int rc_ = fail(nullptr, MSL_ERR_INVALID, "msl_create: stored spectrum %d x %d is not a multiple of the bin %d x %d", h->wx, h->wy, h->bx, h->by);
        delete h; return rc_;
    }
    h->wpix = (size_t)(h->wx / h->bx) * (h->wy / h->by);
    // every (probe, frame) image of the results starts on a 256-byte boundary: the time kernels read 128-byte row segments of
    // neighbouring pixels of every frame, and with an odd pixel count (501 x 491: 245 991) all but one frame in 16 straddled two lines
    h->wpitch = dbg_env("MSL_NO_RESULT_PITCH") ? h->wpix : ((h->wpix + 31) & ~(size_t)31);
    auto bail = [&](int rc) { g_create_error = h->err; msl_destroy(h); return rc; };
    if (hipSetDevice(cfg->device) != hipSuccess) return bail(fail(h, MSL_ERR_HIP, "hipSetDevice(%d) failed", cfg->device));
    if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) return bail(fail(h, MSL_ERR_HIP, "hipStreamCreate failed"));
    allow_lds(h, line_fft_kernel<0, false>);
    allow_lds(h, line_fft_kernel<1, false>);
    allow_lds(h, line_fft_kernel<1, true>);
    allow_lds(h, line_fft_kernel<2, false>);
    allow_lds(h, line_fft_kernel<2, true>);
    int rc;
    {   // the lane <-> register exchange of every register kernel rests on inline asm the compiler cannot check: test it once per process
        static int exchange_ok = -1;
        if (exchange_ok < 0) exchange_ok = rowT_selftest(h->stream);
        if (exchange_ok != 0) return bail(fail(h, MSL_ERR_HIP, "msl_create: the add-tid LDS exchange self-test failed on this device / toolchain (%d values wrong)", exchange_ok));
    }
    if ((rc = make_plan(h, h->plan_x, cfg->nx))) return bail(rc);
    if ((rc = make_plan(h, h->plan_y, cfg->ny))) return bail(rc);
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, cfg->device) == hipSuccess && prop.multiProcessorCount > 0) h->n_cus = prop.multiProcessorCount;
    }
    if (cfg->fft_path == 0) {
        // row kernel: rows of length ny, 256/R rows per workgroup;  column kernel: columns of length nx, 16 per tile
        int ry = fast_radix(cfg->ny), rx = fast_radix(cfg->nx);
        if (ry && cfg->nx % (256 / ry) == 0) { h->Ry = ry; if ((rc = make_tw4(h, h->tw4_y, ry))) return bail(rc); }
        if (rx && cfg->ny % 16 == 0 && cfg->ny >= 32) { h->Rx = rx; if ((rc = make_tw4(h, h->tw4_x, rx))) return bail(rc); }
        { const char* e = dbg_env("MSL_ROW_PCHUNK"); if (e) h->row_pchunk = atoi(e); }
        allow_lds(h, row_pass_pf_kernel<32>);
        allow_lds(h, row_pass_pf_kernel<16>);
        allow_lds(h, col_pass_kernel<32>);
        allow_lds(h, col_pass_kernel<16>);
    }
    const size_t npix = (size_t)cfg->nx * cfg->ny;
    {
        const char* e = dbg_env("MSL_PITCH_PAD");
        int pad = e ? atoi(e) : 16;
        if (pad < 0 || (pad & 1)) pad = 16;
        h->pitch = cfg->ny + ((h->Rx || h->Ry) ? pad : 0);
    }
    {
        const char* e = dbg_env("MSL_SLICE_PATH");           // 2 = force the two-pass four-step loop
        const bool want = cfg->fft_path == 0 && !(e && atoi(e) == 2);
        plan_axis_kind(h, h->opx, cfg->nx, cfg->ny, h->Rx, h->plan_x.M, want);
        plan_axis_kind(h, h->opy, cfg->ny, cfg->nx, h->Ry, h->plan_y.M, want);
        if ((rc = make_axis_tables(h, h->opx, h->opy)) || (rc = make_axis_tables(h, h->opy, h->opx))) return bail(rc);
        h->onepass = h->onepass_planned = h->opx.base != AX_NONE && h->opy.base != AX_NONE;
        h->scheme_b = h->onepass && !(h->opx.kind == AX_FOURSTEP && h->opy.kind == AX_FOURSTEP);
        if (h->pitch == cfg->ny && h->onepass) h->pitch = cfg->ny + 16;        // pad the work buffers of 2R^2 grids too
        if (h->onepass && (h->pitch & 1)) ++h->pitch;                          // even pitches: the transposed stores write two lines (16 bytes) at a time
        if (h->onepass) {
            h->pitchT = cfg->nx + 16 + (cfg->nx & 1);
            if (h->pitch - cfg->ny > 16 && !(cfg->nx & 1)) h->pitchT = cfg->nx + (h->pitch - cfg->ny);
            // transposed probes: only when the first pass runs along x (alternating scheme with an even slice count)
            h->need_psi0T = !h->scheme_b && (cfg->nz % 2 == 0);
        }
        if ((rc = alloc_probe_buffers(h, cfg->n_probes))) return bail(rc);
        if (h->onepass) {
            if ((rc = h->transT.alloc(h, npix * cfg->nz * h->FB))) return bail(rc);
            { const char* ev = dbg_env("MSL_DEBUG_FLAGS_MASK"); if (ev) h->debug_flags_mask = atoi(ev); }
            allow_lds(h, row_pass2_kernel<32>);
            allow_lds(h, row_pass2_kernel<16>);
        }
    }
    if ((rc = h->trans.alloc(h, npix * cfg->nz * h->FB))) return bail(rc);
    if (cfg->keep_potential && (rc = h->V.alloc(h, npix * cfg->nz))) return bail(rc);
    h->pot_ifft = plan_pot_ifft(h);
    if (cfg->n_frames > 0) {
        if ((h->bx > 1 || h->by > 1) && (rc = h->bin_stage.alloc(h, (size_t)h->wx * h->wy * cfg->n_probes * h->FB))) return bail(rc);
        if ((rc = h->layers.alloc(h, layer_block_elems(h)))) return bail(rc);           // a single block: the exit waves
        h->wf = h->layers;
        if (hipMemsetAsync(h->wf, 0, layer_block_elems(h) * sizeof(float2), h->stream) != hipSuccess)
            return bail(fail(h, MSL_ERR_HIP, "memset failed"));
    }
    if ((rc = h->pxt.alloc(h, (size_t)cfg->nx)) || (rc = h->pyt.alloc(h, (size_t)cfg->ny)) || (rc = h->tap_cx.alloc(h, (size_t)cfg->nx)) ||
        (rc = h->tap_cy.alloc(h, (size_t)cfg->ny)) || (rc = h->d_lo.alloc(h, (size_t)cfg->nz)) || (rc = h->d_hi.alloc(h, (size_t)cfg->nz)) ||
        (rc = h->d_abcd.alloc(h, (size_t)103 * 12)) || (rc = h->d_z2s.alloc(h, (size_t)104)) || (rc = h->d_species.alloc(h, (size_t)104)) ||
        (rc = refresh_propagator(h))) return bail(rc);
    *out = h;
    return MSL_OK;
}

int msl_destroy(msl_handle* h) {
    if (!h) return MSL_OK;
    (void)hipSetDevice(h->cfg.device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    for (auto& s : h->ring) for (auto e : s.ev) (void)hipEventDestroy(e);
    for (auto& st : h->stage) { if (st.ev) (void)hipEventDestroy(st.ev); if (st.buf) (void)hipHostFree(st.buf); }
    for (auto e : h->sm_ev) if (e) (void)hipEventDestroy(e);
    const hipStream_t stream = h->stream;
    delete h;                                               // the stream is idle: every DevBuf of the handle frees its memory
    if (stream) (void)hipStreamDestroy(stream);
    return MSL_OK;
}

int msl_set_kirkland(msl_handle* h, const double* abcd) {
    if (!h || !abcd) return fail(h, MSL_ERR_INVALID, "msl_set_kirkland: null argument");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipMemcpyAsync(h->d_abcd, abcd, 103 * 12 * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->have_kirkland = true;
    h->n_species = 0;
    h->ff_n = 0;
    return MSL_OK;
}

int msl_set_slices(msl_handle* h, const double* lo, const double* hi) {
    if (!h || !lo || !hi) return fail(h, MSL_ERR_INVALID, "msl_set_slices: null argument");
    for (int s = 0; s < h->cfg.nz; ++s)
        if (!(hi[s] > lo[s]) || (s > 0 && lo[s] < lo[s - 1]))
            return fail(h, MSL_ERR_INVALID, "msl_set_slices: edges must be increasing with hi>lo (slice %d)", s);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipMemcpyAsync(h->d_lo, lo, h->cfg.nz * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->d_hi, hi, h->cfg.nz * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->h_lo.assign(lo, lo + h->cfg.nz);
    h->h_hi.assign(hi, hi + h->cfg.nz);
    h->have_slices = true;
    return MSL_OK;
}

// finite projection
int msl_set_projection(msl_handle* h, int32_t reach_slices, int32_t nodes) {
    if (!h) return fail(h, MSL_ERR_INVALID, "msl_set_projection: null handle");
    if (nodes < 1 || nodes > 16) return fail(h, MSL_ERR_INVALID, "msl_set_projection: %d nodes per slice outside [1, 16]", nodes);
    if (reach_slices < 0 || reach_slices > 32) return fail(h, MSL_ERR_INVALID, "msl_set_projection: a reach of %d slices outside [0, 32]", reach_slices);
    if (reach_slices > 0 && (h->abs_on || h->tds_on))
        return fail(h, MSL_ERR_UNSUPPORTED, "msl_set_projection: absorptive and TDS tables are not built under finite projection");
    if (reach_slices > 0 && h->ion_on)
        return fail(h, MSL_ERR_UNSUPPORTED, "msl_set_projection: the ionisation weights are not built under finite projection");
    if (reach_slices == h->fin_R && (reach_slices == 0 || nodes == h->fin_J)) { h->fin_J = nodes; return MSL_OK; }     // nothing changes
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipStreamSynchronize(h->stream));          // a queued build still reads the tables
    h->fin_R = reach_slices; h->fin_J = nodes;
    h->pg_valid = false;
    h->ff_n = 0;                                         // d_ff holds f or the channel tables: the next build makes its table again
    return MSL_OK;
}

int msl_get_projection(const msl_handle* h, int32_t* reach_nodes) {
    if (!h || !reach_nodes) return MSL_ERR_INVALID;
    reach_nodes[0] = h->fin_R; reach_nodes[1] = h->fin_J;
    return MSL_OK;
}

int msl_resize_probes(msl_handle* h, int32_t n_probes) {
    if (!h) return fail(h, MSL_ERR_INVALID, "null handle");
    if (n_probes < 1) return fail(h, MSL_ERR_INVALID, "msl_resize_probes: need at least one probe");
    if (h->wf && n_probes != h->cfg.n_probes) return fail(h, MSL_ERR_STATE, "msl_resize_probes: handle owns a (P,T,nx,ny) result buffer");
    if (n_probes == h->cfg.n_probes) return MSL_OK;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    const int rc = alloc_probe_buffers(h, n_probes);
    if (rc) return rc;
    h->cfg.n_probes = n_probes;
    h->have_probes = false; h->have_exit = false;
    h->pm_valid = false; h->pm_g = 0;
    return MSL_OK;
}

int msl_shift_probes(msl_handle* h, const float* base, const double* xy, int32_t n_probes) {
    if (!h || !base || !xy) return fail(h, MSL_ERR_INVALID, "msl_shift_probes: null argument");
    if (n_probes != h->cfg.n_probes) return fail(h, MSL_ERR_INVALID, "msl_shift_probes: %d probes, handle has %d", n_probes, h->cfg.n_probes);
    const msl_config& c = h->cfg;
    HIPCHK(h, hipSetDevice(c.device));
    h->pm_valid = false;                                 // an array probe has no recipe to differentiate
    const size_t npix = (size_t)c.nx * c.ny;
    DevBuf<float2> bk;
    int rc = bk.alloc(h, npix);
    if (rc) return rc;
    HIPCHK(h, hipMemcpyAsync(bk, base, npix * sizeof(float2), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->d_xy, xy, 2 * sizeof(double) * n_probes, hipMemcpyHostToDevice, h->stream));
    h->cur = nullptr;
    rc = fft2_inplace(h, bk, 1, +1, 1.0f, c.ny);
    if (rc == MSL_OK) {
        const long long total = (long long)npix * n_probes;
        hipLaunchKernelGGL(probe_ramp_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->stream, h->psi0, bk, h->d_xy,
                           n_probes, c.nx, c.ny, h->pitch, 1.0 / (c.nx * c.dx), 1.0 / (c.ny * c.dy));
        if (hipGetLastError() != hipSuccess) rc = fail(h, MSL_ERR_HIP, "probe_ramp_kernel launch failed");
    }
    if (rc == MSL_OK) rc = fft2_inplace(h, h->psi0, n_probes, -1, 1.0f / ((float)c.nx * (float)c.ny), h->pitch);
    if (rc == MSL_OK) rc = transpose_probes(h);
    hipError_t e = hipStreamSynchronize(h->stream);
    if (rc) return rc;
    if (e != hipSuccess) return fail(h, MSL_ERR_HIP, "msl_shift_probes: %s", hipGetErrorString(e));
    h->have_probes = true;
    return MSL_OK;
}

int msl_set_aberrations(msl_handle* h, const double* polar, int32_t n_terms) {
    if (!h) return fail(h, MSL_ERR_INVALID, "null handle");
    h->pm_valid = false;                                 // the probes on the device are those of the earlier coefficients
    if (n_terms == 0) {
        memset(h->aberr_polar, 0, sizeof(h->aberr_polar));
        h->have_aberr = false;
        return MSL_OK;
    }
    if (n_terms != 14) return fail(h, MSL_ERR_INVALID, "msl_set_aberrations: %d terms, need 14 (or 0 to clear)", n_terms);
    if (!polar) return fail(h, MSL_ERR_INVALID, "msl_set_aberrations: null argument");
    bool any = false;
    for (int k = 0; k < 28; ++k) {
        if (!std::isfinite(polar[k])) return fail(h, MSL_ERR_INVALID, "msl_set_aberrations: value %d is not finite", k);
        if (!(k & 1) && polar[k] != 0) any = true;
    }
    memcpy(h->aberr_polar, polar, sizeof(h->aberr_polar));
    h->have_aberr = any;
    return MSL_OK;
}

// the tail of every call that fills the probe buffer: the transposed copy the slice loop starts from, one wait, the flag
static int finish_probes(msl_handle* h) {
    h->pm_valid = false;                                 // (msl_set_probes sets it again behind this)
    int rc = transpose_probes(h);
    if (rc) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->have_probes = true;
    return MSL_OK;
}

// ... of msl_set_probes and msl_set_probe_members, whose kernel has just been queued: reciprocal-space probes to real space first
static int finish_kspace_probes(msl_handle* h, int32_t n_probes) {
    HIPCHK(h, hipGetLastError());
    const int rc = fft2_inplace(h, h->psi0, n_probes, -1, 1.0f / ((float)h->cfg.nx * (float)h->cfg.ny), h->pitch);
    return rc ? rc : finish_probes(h);
}

int msl_set_probes(msl_handle* h, double mrad, const double* xy, int32_t n_probes) {
    if (!h || !xy) return fail(h, MSL_ERR_INVALID, "msl_set_probes: null argument");
    if (n_probes != h->cfg.n_probes) return fail(h, MSL_ERR_INVALID, "msl_set_probes: %d probes, handle has %d", n_probes, h->cfg.n_probes);
    if (mrad < 0) return fail(h, MSL_ERR_INVALID, "msl_set_probes: negative aperture");
    const msl_config& c = h->cfg;
    HIPCHK(h, hipSetDevice(c.device));
    HIPCHK(h, hipMemcpyAsync(h->d_xy, xy, 2 * sizeof(double) * n_probes, hipMemcpyHostToDevice, h->stream));
    const long long total = (long long)c.nx * c.ny * n_probes;
    const double lx = c.nx * c.dx, ly = c.ny * c.dy;
    if (h->have_aberr && mrad != 0) {
        hipLaunchKernelGGL(probe_kspace_aberr_kernel<false>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->stream, h->psi0, h->d_xy,
                           (const double*)nullptr, n_probes, c.nx, c.ny, h->pitch, 1.0 / lx, 1.0 / ly, 1.0 / (c.nx * c.dx), 1.0 / (c.ny * c.dy),
                           (mrad * 1e-3) / c.wavelength, c.wavelength, probe_aberrations(h->aberr_polar[0], c.wavelength));
    } else {
        hipLaunchKernelGGL(probe_kspace_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->stream, h->psi0, h->d_xy,
                           n_probes, c.nx, c.ny, h->pitch, 1.0 / lx, 1.0 / ly, 1.0 / (c.nx * c.dx), 1.0 / (c.ny * c.dy),
                           (mrad * 1e-3) / c.wavelength, mrad == 0 ? 1 : 0);
    }
    const int rc = finish_kspace_probes(h, n_probes);
    if (rc == MSL_OK && mrad > 0) {                      // the recipe of these probes, for msl_adjoint_probe_params
        h->pm_mrad = mrad; h->pm_wavelength = c.wavelength;
        if (h->have_aberr) h->pm_ab = probe_aberrations(h->aberr_polar[0], c.wavelength);
        else h->pm_ab = ProbeAberrations{};
        // the positions on the device, a copy of the chain's own: d_xy is rewritten by calls that do not touch the probe buffer
        int rc2 = h->pm_dxy.reserve(h, (size_t)2 * n_probes);
        if (rc2) return rc2;
        HIPCHK(h, hipMemcpyAsync(h->pm_dxy, h->d_xy, (size_t)2 * n_probes * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        h->pm_valid = true;
    }
    return rc;
}

int msl_set_probe_members(msl_handle* h, double mrad, const double* xy, const double* defocus, int32_t n_probes) {
    if (!h || !xy || !defocus) return fail(h, MSL_ERR_INVALID, "msl_set_probe_members: null argument");
    if (n_probes != h->cfg.n_probes) return fail(h, MSL_ERR_INVALID, "msl_set_probe_members: %d probes, handle has %d", n_probes, h->cfg.n_probes);
    if (mrad < 0) return fail(h, MSL_ERR_INVALID, "msl_set_probe_members: negative aperture");
    if (mrad == 0) return fail(h, MSL_ERR_INVALID, "msl_set_probe_members: plane waves (mrad == 0) have no defocus");
    bool any = false;
    for (int p = 0; p < n_probes; ++p) {
        if (!std::isfinite(defocus[p])) return fail(h, MSL_ERR_INVALID, "msl_set_probe_members: defocus %d is not finite", p);
        if (defocus[p] != 0) any = true;
    }
    if (!any) {                                                 // every member at the handle's own C10: that call, bit for bit
        const int rc0 = msl_set_probes(h, mrad, xy, n_probes);
        h->pm_valid = false;                                    // (member probes are not differentiated)
        return rc0;
    }
    const msl_config& c = h->cfg;
    HIPCHK(h, hipSetDevice(c.device));
    int rc = h->mem_a0.reserve(h, (size_t)n_probes);
    if (rc) return rc;
    // the C10 coefficient of probe p is (C10 + defocus[p]) / (2 lambda), every other one is the handle's
    std::vector<double> a0((size_t)n_probes);
    for (int p = 0; p < n_probes; ++p) a0[p] = (h->aberr_polar[0][0] + defocus[p]) / (2 * c.wavelength);
    HIPCHK(h, hipMemcpyAsync(h->d_xy, xy, 2 * sizeof(double) * n_probes, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->mem_a0.p, a0.data(), sizeof(double) * n_probes, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));                 // (a0 is this call's own: copied before it goes)
    const long long total = (long long)c.nx * c.ny * n_probes;
    const double lx = c.nx * c.dx, ly = c.ny * c.dy;
    hipLaunchKernelGGL(probe_kspace_aberr_kernel<true>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->stream, h->psi0, h->d_xy,
                       (const double*)h->mem_a0.p, n_probes, c.nx, c.ny, h->pitch, 1.0 / lx, 1.0 / ly, 1.0 / (c.nx * c.dx), 1.0 / (c.ny * c.dy),
                       (mrad * 1e-3) / c.wavelength, c.wavelength, probe_aberrations(h->aberr_polar[0], c.wavelength));
    return finish_kspace_probes(h, n_probes);
}

int msl_upload_probes(msl_handle* h, const float* c64, int32_t n_probes) {
    if (!h || !c64) return fail(h, MSL_ERR_INVALID, "msl_upload_probes: null argument");
    if (n_probes != h->cfg.n_probes) return fail(h, MSL_ERR_INVALID, "msl_upload_probes: %d probes, handle has %d", n_probes, h->cfg.n_probes);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipMemcpy2DAsync(h->psi0, (size_t)h->pitch * sizeof(float2), c64, (size_t)h->cfg.ny * sizeof(float2),
                               (size_t)h->cfg.ny * sizeof(float2), (size_t)n_probes * h->cfg.nx, hipMemcpyHostToDevice, h->stream));
    return finish_probes(h);
}

static int check_potential_args(msl_handle* h, const char* who, const double* pos, const int32_t* Z, int64_t n, int32_t ax1, int32_t ax2, int32_t axs) {
    if (!h || (n > 0 && (!pos || !Z))) return fail(h, MSL_ERR_INVALID, "%s: null argument", who);
    if (!h->have_kirkland) return fail(h, MSL_ERR_STATE, "%s: call msl_set_kirkland first", who);
    if (!h->have_slices) return fail(h, MSL_ERR_STATE, "%s: call msl_set_slices first", who);
    if (n < 0 || n > 0x7fffffff) return fail(h, MSL_ERR_INVALID, "%s: bad atom count", who);
    if (ax1 < 0 || ax1 > 2 || ax2 < 0 || ax2 > 2 || axs < 0 || axs > 2 || ((1 << ax1) | (1 << ax2) | (1 << axs)) != 7)
        return fail(h, MSL_ERR_INVALID, "%s: axes must be a permutation of 0,1,2", who);
    return MSL_OK;
}

int msl_build_potential(msl_handle* h, const double* pos, const int32_t* Z, int64_t n, int32_t ax1, int32_t ax2, int32_t axs) {
    int rc = check_potential_args(h, "msl_build_potential", pos, Z, n, ax1, ax2, axs);
    if (rc) return rc;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    return build_potentials(h, pos, Z, n, 1, h->cur_batch, ax1, ax2, axs);
}

int msl_build_potentials(msl_handle* h, const double* pos, const int32_t* Z, int64_t n, int32_t count, int32_t ax1, int32_t ax2, int32_t axs) {
    int rc = check_potential_args(h, "msl_build_potentials", pos, Z, n, ax1, ax2, axs);
    if (rc) return rc;
    if (count < 1 || count > h->FB) return fail(h, MSL_ERR_INVALID, "msl_build_potentials: count %d outside [1,%d] (msl_config.frame_batch)", count, h->FB);
    if ((int64_t)n * count > 0x7fffffffLL) return fail(h, MSL_ERR_INVALID, "msl_build_potentials: more than 2^31 atoms in one batch");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    rc = build_potentials(h, pos, Z, n, count, 0, ax1, ax2, axs);
    if (rc == MSL_OK) h->cur_batch = count - 1;         // the current stack (MSL_BUF_TRANSMISSION, msl_propagate) is the last frame's, as after `count` single builds
    return rc;
}

// ---- frozen phonons ----------------------------------------------------------
int msl_set_structure(msl_handle* h, const double* pos0, const int32_t* Z, const double* sigma, int64_t n, int32_t ax1, int32_t ax2, int32_t axs) {
    if (!h || (n > 0 && (!pos0 || !Z || !sigma))) return fail(h, MSL_ERR_INVALID, "msl_set_structure: null argument");
    if (n < 0 || n > 0x7fffffff) return fail(h, MSL_ERR_INVALID, "msl_set_structure: bad atom count");
    if (ax1 < 0 || ax1 > 2 || ax2 < 0 || ax2 > 2 || axs < 0 || axs > 2 || ((1 << ax1) | (1 << ax2) | (1 << axs)) != 7)
        return fail(h, MSL_ERR_INVALID, "msl_set_structure: axes must be a permutation of 0,1,2");
    PotGroup m{};
    for (int i = 0; i < 104; ++i) m.z2s[i] = -1;
    for (int64_t a = 0; a < n; ++a) {
        if (Z[a] < 1 || Z[a] > 103) return fail(h, MSL_ERR_INVALID, "msl_set_structure: atomic number %d out of 1..103", Z[a]);
        if (!(sigma[a] >= 0.0) || !std::isfinite(sigma[a]))
            return fail(h, MSL_ERR_INVALID, "msl_set_structure: width %g of atom %lld is not a finite number >= 0", sigma[a], (long long)a);
        m.z2s[Z[a]] = 0;
    }
    m.nsp = 0;
    for (int z = 1; z <= 103; ++z) if (m.z2s[z] == 0) { m.z2s[z] = m.nsp; m.species[m.nsp++] = z; }
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipStreamSynchronize(h->stream));          // a build queued from the previous structure still reads its buffers
    h->have_structure = false;
    drop_modes(h);                                       // they belong to the atoms of the structure they were set on
    int rc;
    if ((rc = h->th_pos0.alloc(h, (size_t)n * 3)) || (rc = h->th_sigma.alloc(h, (size_t)n)) || (rc = h->th_Z.alloc(h, (size_t)n)) ||
        (rc = h->th_z2s.alloc(h, (size_t)104)) || (rc = h->th_species.alloc(h, (size_t)104))) return rc;
    if (n > 0) {
        HIPCHK(h, hipMemcpy(h->th_pos0, pos0, (size_t)n * 3 * sizeof(double), hipMemcpyHostToDevice));
        HIPCHK(h, hipMemcpy(h->th_sigma, sigma, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
        HIPCHK(h, hipMemcpy(h->th_Z, Z, (size_t)n * sizeof(int), hipMemcpyHostToDevice));
    }
    HIPCHK(h, hipMemcpy(h->th_z2s, m.z2s, sizeof m.z2s, hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(h->th_species, m.species, sizeof m.species, hipMemcpyHostToDevice));
    memcpy(h->th_map_z2s, m.z2s, sizeof m.z2s);
    memcpy(h->th_map_species, m.species, sizeof m.species);
    h->th_nsp = m.nsp; h->th_n = n; h->th_ax1 = ax1; h->th_ax2 = ax2; h->th_axs = axs;
    h->have_structure = true;
    return MSL_OK;
}

// msl_build_thermal / msl_build_modes: the state and count checks, then build_potentials on the generated source
static int build_generated(msl_handle* h, const char* who, bool modes, uint64_t seed, int64_t first, int32_t count) {
    if (!h) return fail(h, MSL_ERR_INVALID, "%s: null handle", who);
    if (h->abs_on) return fail(h, MSL_ERR_STATE, "%s: absorption is set (msl_set_absorption): the vibration would be counted twice", who);
    if (!h->have_structure) return fail(h, MSL_ERR_INVALID, "%s: no structure (call msl_set_structure first)", who);
    if (modes && !h->have_modes) return fail(h, MSL_ERR_INVALID, "%s: no modes (call msl_set_modes first)", who);
    if (!h->have_kirkland) return fail(h, MSL_ERR_STATE, "%s: call msl_set_kirkland first", who);
    if (!h->have_slices) return fail(h, MSL_ERR_STATE, "%s: call msl_set_slices first", who);
    if (count < 1 || count > h->FB) return fail(h, MSL_ERR_INVALID, "%s: count %d outside [1,%d] (msl_config.frame_batch)", who, count, h->FB);
    if (first < 0 || first > INT64_MAX - count)
        return fail(h, MSL_ERR_INVALID, "%s: %s %lld .. outside [0, 2^63)", who, modes ? "frames" : "configurations", (long long)first);
    if (modes && h->md_dynamic && first + count > (1LL << 31))
        return fail(h, MSL_ERR_INVALID, "%s: frames %lld .. %lld of a dynamic record outside [0, 2^31)", who, (long long)first, (long long)(first + count - 1));
    if (h->th_n * count > 0x7fffffffLL) return fail(h, MSL_ERR_INVALID, "%s: more than 2^31 atoms in one batch", who);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const GeneratedSource src{modes, seed, (uint64_t)first};
    // a frame batch of 1: the selected slot, as msl_build_potential; else the slots 0 .. count-1, as msl_build_potentials
    const int first_slot = h->FB > 1 ? 0 : h->cur_batch;
    int rc = build_potentials(h, nullptr, nullptr, h->th_n, count, first_slot, h->th_ax1, h->th_ax2, h->th_axs, &src);
    if (rc == MSL_OK && h->FB > 1) h->cur_batch = count - 1;
    return rc;
}

int msl_build_thermal(msl_handle* h, uint64_t seed, int64_t first_config, int32_t count) {
    return build_generated(h, "msl_build_thermal", false, seed, first_config, count);
}

int msl_thermal_positions(msl_handle* h, uint64_t seed, int64_t config, double* out) {
    if (!h) return fail(h, MSL_ERR_INVALID, "msl_thermal_positions: null handle");
    if (!h->have_structure) return fail(h, MSL_ERR_INVALID, "msl_thermal_positions: no structure (call msl_set_structure first)");
    if (config < 0) return fail(h, MSL_ERR_INVALID, "msl_thermal_positions: configuration %lld is negative", (long long)config);
    const int64_t n = h->th_n;
    if (n == 0) return MSL_OK;
    if (!out) return fail(h, MSL_ERR_INVALID, "msl_thermal_positions: null argument");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    DevBuf<double> tmp;                                   // (not d_pos: a queued build may still read it)
    int rc = tmp.alloc(h, (size_t)n * 3);
    if (rc) return rc;
    hipLaunchKernelGGL(thermal_positions_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, h->th_pos0, h->th_sigma,
                       (long long)n, 1, (unsigned long long)seed, (unsigned long long)config, tmp.p);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(out, tmp, (size_t)n * 3 * sizeof(double), hipMemcpyDeviceToHost, h->stream);
    const hipError_t es = hipStreamSynchronize(h->stream);      // on every path: nothing queued reads tmp when it is freed below
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return fail(h, MSL_ERR_HIP, "msl_thermal_positions failed: %s", hipGetErrorString(e));
    return MSL_OK;
}

// ---- phonon modes ------------------------------------------------------------
int msl_set_modes(msl_handle* h, const int32_t* basis_index, int64_t n_atoms, int32_t n_basis, const double* q, const double* tau,
                  const double* W, int32_t n_modes, int32_t dynamic) {
    if (!h) return fail(h, MSL_ERR_INVALID, "msl_set_modes: null handle");
    if (!h->have_structure) return fail(h, MSL_ERR_INVALID, "msl_set_modes: no structure (call msl_set_structure first)");
    if (n_atoms != h->th_n)
        return fail(h, MSL_ERR_INVALID, "msl_set_modes: %lld atoms, the structure has %lld", (long long)n_atoms, (long long)h->th_n);
    if (n_modes < 1) return fail(h, MSL_ERR_INVALID, "msl_set_modes: n_modes %d is below 1", n_modes);
    if (n_basis < 1) return fail(h, MSL_ERR_INVALID, "msl_set_modes: n_basis %d is below 1", n_basis);
    if (!q || !tau || !W || (n_atoms > 0 && !basis_index)) return fail(h, MSL_ERR_INVALID, "msl_set_modes: null argument");
    const size_t M = (size_t)n_modes, nW = M * (size_t)n_basis * 6;
    if ((long long)n_modes * h->FB > 0x7fffffffLL) return fail(h, MSL_ERR_INVALID, "msl_set_modes: n_modes x frame_batch exceeds 2^31");
    if (nW > (size_t)1 << 40) return fail(h, MSL_ERR_INVALID, "msl_set_modes: n_modes x n_basis is too large");
    for (int64_t a = 0; a < n_atoms; ++a)
        if (basis_index[a] < 0 || basis_index[a] >= n_basis)
            return fail(h, MSL_ERR_INVALID, "msl_set_modes: basis index %d of atom %lld outside [0,%d)", basis_index[a], (long long)a, n_basis);
    for (size_t m = 0; m < M; ++m) {
        if (!std::isfinite(tau[m]) || !(tau[m] >= 0.0))
            return fail(h, MSL_ERR_INVALID, "msl_set_modes: tau %g of mode %zu is not a finite number >= 0", tau[m], m);
        if (!std::isfinite(q[m * 3]) || !std::isfinite(q[m * 3 + 1]) || !std::isfinite(q[m * 3 + 2]))
            return fail(h, MSL_ERR_INVALID, "msl_set_modes: wave vector of mode %zu is not finite", m);
    }
    for (size_t k = 0; k < nW; ++k)
        if (!std::isfinite(W[k])) return fail(h, MSL_ERR_INVALID, "msl_set_modes: displacement vector of mode %zu is not finite", k / ((size_t)n_basis * 6));
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipStreamSynchronize(h->stream));          // a build queued from the previous modes still reads their buffers
    drop_modes(h);
    int rc;
    if ((rc = h->md_basis.alloc(h, (size_t)n_atoms)) || (rc = h->md_q.alloc(h, M * 3)) || (rc = h->md_tau.alloc(h, M)) ||
        (rc = h->md_W.alloc(h, nW)) || (rc = h->md_C.alloc(h, M * (size_t)std::max(1, h->FB)))) { drop_modes(h); return rc; }
    if (n_atoms > 0) HIPCHK(h, hipMemcpy(h->md_basis, basis_index, (size_t)n_atoms * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(h->md_q, q, M * 3 * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(h->md_tau, tau, M * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(h->md_W, W, nW * sizeof(double), hipMemcpyHostToDevice));
    h->md_M = n_modes; h->md_nb = n_basis; h->md_dynamic = dynamic != 0;
    h->have_modes = true;
    return MSL_OK;
}

// ---- per-slice sums: TDS detector signal and element maps (DESIGN.md sections 4.23, 4.27; msl_set_absorption, msl_set_tds and
// msl_set_ionization stand with the handle settings; slice_sums_fetch and slice_sums_reduce with the queue) ----
int msl_tds_fetch(msl_handle* h, int32_t B, double* out) {
    if (!h || !out) return fail(h, MSL_ERR_INVALID, "msl_tds_fetch: null argument");
    if (!h->tds_on || !h->tds_have) return fail(h, MSL_ERR_STATE, "msl_tds_fetch: no TDS sums (msl_set_tds, then a slice loop)");
    int rc = slice_sums_fetch(h, "msl_tds_fetch", h->tds_acc, h->tds_n, &B, out);
    if (rc) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return MSL_OK;
}

int msl_tds_reduce(msl_handle* h, int32_t slice, int32_t reps, double* out, double* ms_reduce) {
    return slice_sums_reduce<TdsSignal>(h, "msl_tds_reduce", slice, reps, out, ms_reduce);
}

int msl_ionization_fetch(msl_handle* h, int32_t B, double* out) {
    if (!h || !out) return fail(h, MSL_ERR_INVALID, "msl_ionization_fetch: null argument");
    if (!h->ion_on || !h->ion_have) return fail(h, MSL_ERR_STATE, "msl_ionization_fetch: no sums (msl_set_ionization, then a slice loop)");
    const int n = h->ion_n, nz = h->cfg.nz;
    int rc = slice_sums_fetch(h, "msl_ionization_fetch", h->ion_acc, n, &B, out);
    if (rc) return rc;
    std::vector<double> norm((size_t)B);
    HIPCHK(h, hipMemcpyAsync(norm.data(), h->ion_norm, (size_t)B * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (int z = 0; z < nz; ++z)                            // per incident electron: over the norm of the probe, in float64
        for (int p = 0; p < B; ++p)
            for (int e = 0; e < n; ++e) out[((size_t)z * B + p) * n + e] /= norm[p];
    return MSL_OK;
}

int msl_ionization_reduce(msl_handle* h, int32_t slice, int32_t reps, double* out, double* ms_reduce) {
    return slice_sums_reduce<IonSignal>(h, "msl_ionization_reduce", slice, reps, out, ms_reduce);
}

int msl_build_modes(msl_handle* h, uint64_t seed, int64_t first_frame, int32_t count) {
    return build_generated(h, "msl_build_modes", true, seed, first_frame, count);
}

int msl_mode_positions(msl_handle* h, uint64_t seed, int64_t frame, double* out) {
    if (!h) return fail(h, MSL_ERR_INVALID, "msl_mode_positions: null handle");
    if (!h->have_structure) return fail(h, MSL_ERR_INVALID, "msl_mode_positions: no structure (call msl_set_structure first)");
    if (!h->have_modes) return fail(h, MSL_ERR_INVALID, "msl_mode_positions: no modes (call msl_set_modes first)");
    if (frame < 0 || (h->md_dynamic && frame >= (1LL << 31)))
        return fail(h, MSL_ERR_INVALID, "msl_mode_positions: frame %lld outside [0, %s)", (long long)frame, h->md_dynamic ? "2^31" : "2^63");
    const int64_t n = h->th_n;
    if (n == 0) return MSL_OK;
    if (!out) return fail(h, MSL_ERR_INVALID, "msl_mode_positions: null argument");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    DevBuf<double> tmp;                                   // (not d_pos: a queued build may still read it)
    int rc = tmp.alloc(h, (size_t)n * 3);
    if (rc) return rc;
    rc = launch_mode_positions(h, n, 1, seed, (uint64_t)frame, tmp.p);
    hipError_t e = hipSuccess;
    if (rc == MSL_OK) e = hipMemcpyAsync(out, tmp, (size_t)n * 3 * sizeof(double), hipMemcpyDeviceToHost, h->stream);
    const hipError_t es = hipStreamSynchronize(h->stream);      // on every path: nothing queued reads tmp when it is freed below
    if (rc) return rc;
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return fail(h, MSL_ERR_HIP, "msl_mode_positions failed: %s", hipGetErrorString(e));
    return MSL_OK;
}

int msl_upload_potential(msl_handle* h, const float* V) {
    if (!h || !V) return fail(h, MSL_ERR_INVALID, "msl_upload_potential: null argument");
    const msl_config& c = h->cfg;
    HIPCHK(h, hipSetDevice(c.device));
    const size_t n = (size_t)c.nx * c.ny * c.nz;
    float* dst = h->V;
    DevBuf<float> tmp;
    if (!dst) { int rc = tmp.alloc(h, n); if (rc) return rc; dst = tmp; }
    HIPCHK(h, hipMemcpyAsync(dst, V, n * sizeof(float), hipMemcpyHostToDevice, h->stream));
    int rc = transmission_from_V(h, dst, h->cur_batch);
    if (rc || (rc = finish_stacks(h, h->cur_batch, 1))) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->have_potential = true;
    h->abs_built = false;
    h->pg_valid = false;                                // (nor atoms to differentiate with respect to)
    h->ion_built = false;                               // (an uploaded potential has no atoms to make the ionisation weights from)
    return MSL_OK;
}

// slice loop of `groups` frames whose transmission stacks start at batch slot `first_group`
static int run_loop(msl_handle* h, int slot, int groups, int first_group) {
    if (!h->have_probes) return fail(h, MSL_ERR_STATE, "propagate: no probes (msl_set_probes / msl_upload_probes)");
    if (!h->have_potential) return fail(h, MSL_ERR_STATE, "propagate: no potential (msl_build_potential / msl_upload_potential)");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    // the reduce mode: the exit block is the last layer, reduced behind the epilogue like every tapped one
    const bool reduce = h->lr_on && slot >= 0;
    const bool timed = h->cfg.launch_timing;            // else queued; msl_synchronize / msl_download wait for it
    EventPair timer;
    int rc;
    if ((timed && (rc = timer.begin(h))) || (rc = slice_loop(h, slot, groups, first_group, h->tds_on || h->ion_on))) return rc;
    if (reduce && (rc = layer_reduce_queue(h, n_taps(h), h->wf, slot, groups))) return rc;
    return timed ? timer.end(h, &h->ctr.ms_propagate) : MSL_OK;
}

int msl_propagate(msl_handle* h) {
    if (!h) return fail(h, MSL_ERR_INVALID, "null handle");
    int rc = run_loop(h, -1, 1, h->cur_batch);
    if (rc == MSL_OK) h->have_exit = true;
    return rc;
}

int msl_propagate_frame(msl_handle* h, int32_t slot) {
    if (!h) return fail(h, MSL_ERR_INVALID, "null handle");
    if (!h->wf) return fail(h, MSL_ERR_STATE, "msl_propagate_frame: handle created with n_frames == 0");
    if (slot < 0 || slot >= h->cfg.n_frames) return fail(h, MSL_ERR_INVALID, "msl_propagate_frame: slot %d out of range [0,%d)", slot, h->cfg.n_frames);
    return run_loop(h, slot, 1, h->cur_batch);
}

int msl_select_batch_slot(msl_handle* h, int32_t b) {
    if (!h) return fail(h, MSL_ERR_INVALID, "null handle");
    if (b < 0 || b >= h->FB) return fail(h, MSL_ERR_INVALID, "msl_select_batch_slot: slot %d out of range [0,%d)", b, h->FB);
    h->cur_batch = b;
    return MSL_OK;
}

int msl_frame_batch(const msl_handle* h) { return h ? h->FB : 0; }

int msl_propagate_frames(msl_handle* h, int32_t first_slot, int32_t count) {
    if (!h) return fail(h, MSL_ERR_INVALID, "null handle");
    if (!h->wf) return fail(h, MSL_ERR_STATE, "msl_propagate_frames: handle created with n_frames == 0");
    if (count < 1 || count > h->FB) return fail(h, MSL_ERR_INVALID, "msl_propagate_frames: count %d outside [1,%d] (msl_config.frame_batch)", count, h->FB);
    if (first_slot < 0 || first_slot + count > h->cfg.n_frames)
        return fail(h, MSL_ERR_INVALID, "msl_propagate_frames: slots [%d,%d) outside [0,%d)", first_slot, first_slot + count, h->cfg.n_frames);
    return run_loop(h, first_slot, count, 0);
}

// ---- PRISM: plane-wave S-matrix and probe synthesis (smatrix.h) --------------------------------------------
int msl_smatrix_begin(msl_handle* h, int32_t fx, int32_t fy, double mrad) {
    if (!h) return fail(h, MSL_ERR_INVALID, "msl_smatrix_begin: null handle");
    const msl_config& c = h->cfg;
    if (!(mrad > 0) || !std::isfinite(mrad)) return fail(h, MSL_ERR_INVALID, "msl_smatrix_begin: the aperture must be positive (a plane wave needs no S-matrix)");
    if (fx < 1 || fy < 1 || c.nx % fx || c.ny % fy)
        return fail(h, MSL_ERR_INVALID, "msl_smatrix_begin: interpolation (%d, %d) must be positive and divide the %d x %d grid", fx, fy, c.nx, c.ny);
    HIPCHK(h, hipSetDevice(c.device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    smatrix_release(h);
    // the beams: unshifted pixels inside the aperture (the rule of probe_kspace_kernel) whose signed indices are multiples of f
    const double kfx = 1.0 / (c.nx * c.dx), kfy = 1.0 / (c.ny * c.dy), radius = (mrad * 1e-3) / c.wavelength;
    auto freq = [](int m, int n) { return (m < (n + 1) / 2) ? m : m - n; };
    std::vector<int32_t> hb;
    for (int mx = 0; mx < c.nx; ++mx) {
        const int hx = freq(mx, c.nx);
        if (hx % fx) continue;
        for (int my = 0; my < c.ny; ++my) {
            const int hy = freq(my, c.ny);
            if (hy % fy) continue;
            const double kx = hx * kfx, ky = hy * kfy;
            if (sqrt(kx * kx + ky * ky) < radius) { hb.push_back(hx); hb.push_back(hy); }
        }
    }
    const size_t Bm = hb.size() / 2;                        // >= 1: the beam (0, 0) is inside every positive aperture
    if (Bm > 0x7fffffffull / 2) return fail(h, MSL_ERR_INVALID, "msl_smatrix_begin: %zu beams", Bm);
    int rc;
    if ((rc = h->sm_S.alloc(h, Bm * (size_t)c.nx * c.ny)) || (rc = h->sm_beams.alloc(h, Bm)) || (rc = h->sm_c.alloc(h, Bm * (size_t)c.n_probes))) {
        smatrix_release(h);
        return rc;
    }
    HIPCHK(h, hipMemcpyAsync(h->sm_beams, hb.data(), Bm * sizeof(int2), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->sm_h.swap(hb);
    h->sm_fx = fx; h->sm_fy = fy; h->sm_Bm = (int)Bm;
    h->sm_open = true;
    return MSL_OK;
}

int msl_smatrix_beams(const msl_handle* h, int32_t* hxhy) {
    if (!h) return MSL_ERR_INVALID;
    if (!h->sm_open) return MSL_ERR_STATE;
    if (hxhy) memcpy(hxhy, h->sm_h.data(), h->sm_h.size() * sizeof(int32_t));
    return h->sm_Bm;
}

int msl_smatrix_build(msl_handle* h) {
    if (!h) return fail(h, MSL_ERR_INVALID, "msl_smatrix_build: null handle");
    if (!h->sm_open) return fail(h, MSL_ERR_STATE, "msl_smatrix_build: call msl_smatrix_begin first");
    if (!h->have_potential) return fail(h, MSL_ERR_STATE, "msl_smatrix_build: no potential (msl_build_potential / msl_upload_potential)");
    const msl_config& c = h->cfg;
    HIPCHK(h, hipSetDevice(c.device));
    EventPair timer;
    int rc;
    if (c.launch_timing && (rc = timer.begin(h))) return rc;
    h->have_probes = false; h->have_exit = false; h->sm_built = false;      // the probe and work buffers carry the beams
    h->pm_valid = false; h->pm_g = 0;
    const int P = c.n_probes;
    const long long total = (long long)c.nx * c.ny * P;
    const size_t row = (size_t)c.ny * sizeof(float2);
    for (int b0 = 0; b0 < h->sm_Bm; b0 += P) {
        const int count = std::min(P, h->sm_Bm - b0);
        hipLaunchKernelGGL(plane_wave_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->stream, h->psi0.p, (const int2*)h->sm_beams.p, b0, count, P,
                           c.nx, c.ny, h->pitch);
        HIPCHK(h, hipGetLastError());
        if ((rc = transpose_probes(h)) || (rc = slice_loop(h, -1, 1, h->cur_batch))) return rc;
        // the unfused loop leaves the exit waves in natural order at the work pitch (what msl_download(MSL_BUF_EXIT) reads)
        HIPCHK(h, hipMemcpy2DAsync(h->sm_S + (size_t)b0 * c.nx * c.ny, row, h->psi, (size_t)h->pitch * sizeof(float2), row, (size_t)count * c.nx,
                                   hipMemcpyDeviceToDevice, h->stream));
        h->ctr.algorithmic_bytes += (uint64_t)count * c.nx * c.ny * 16ull;
    }
    h->sm_built = true;
    return c.launch_timing ? timer.end(h, &h->ctr.ms_propagate) : MSL_OK;
}

extern "C++" template <int G>
static void launch_synth(msl_handle* h, bool vec, int win_x, int win_y) {
    const msl_config& c = h->cfg;
    const int lanes_y = vec ? c.ny / 2 : c.ny;
    const dim3 grid((unsigned)((c.n_probes + G - 1) / G), (unsigned)((c.nx + SM_TILE_ROWS - 1) / SM_TILE_ROWS), (unsigned)((lanes_y + SM_TILE_LANES - 1) / SM_TILE_LANES));
    if (vec) hipLaunchKernelGGL((smatrix_synth_kernel<G, true>), grid, dim3(256), 0, h->stream, (const float2*)h->sm_S.p, (const float2*)h->sm_c.p, (const double*)h->d_xy.p,
                                c.n_probes, h->sm_Bm, c.nx, c.ny, h->pitch, win_x, win_y, c.dx, c.dy, h->psi.p, h->psi0.p);
    else hipLaunchKernelGGL((smatrix_synth_kernel<G, false>), grid, dim3(256), 0, h->stream, (const float2*)h->sm_S.p, (const float2*)h->sm_c.p, (const double*)h->d_xy.p,
                            c.n_probes, h->sm_Bm, c.nx, c.ny, h->pitch, win_x, win_y, c.dx, c.dy, h->psi.p, h->psi0.p);
}

// c[p, b] of the n_probes positions in d_xy into sm_c (both hold that many), with the aberrations of the handle: one timed launch
static int smatrix_coefficients(msl_handle* h, int n_probes) {
    const msl_config& c = h->cfg;
    const ProbeAberrations ab = h->have_aberr ? probe_aberrations(h->aberr_polar[0], c.wavelength) : ProbeAberrations{};
    const long long nc = (long long)n_probes * h->sm_Bm;
    const float scale = (float)((double)h->sm_fx * h->sm_fy / ((double)c.nx * c.ny));
    hipLaunchKernelGGL(smatrix_coeff_kernel, dim3((unsigned)((nc + 255) / 256)), dim3(256), 0, h->stream, h->sm_c.p, (const double*)h->d_xy.p,
                       (const int2*)h->sm_beams.p, n_probes, h->sm_Bm, c.nx, c.ny, 1.0 / (c.nx * c.dx), 1.0 / (c.ny * c.dy), 1.0 / (c.nx * c.dx),
                       1.0 / (c.ny * c.dy), c.wavelength, scale, (int)h->have_aberr, ab);
    HIPCHK(h, hipGetLastError());
    return mark_launch(h, K_OTHER);
}

// fftshift(fft2(.)) of the n_probes waves in the probe buffer into the frame slot: the row transform along y, then the exit
// epilogue -- the sequence of the layer tap
static int smatrix_spectra(msl_handle* h, int n_probes, int slot) {
    int rc;
    if (h->Ry) {
        RowJob r = row_job(h, h->psi0, n_probes, h->pitch);
        r.do_fft = true;
        rc = launch_row_fast(h, r, K_OTHER);
    } else {
        LineArgs r = row_args(h, h->psi0, h->psi0, n_probes, h->pitch);
        r.fft1 = +1;
        rc = launch_lines(h, h->plan_y, r, K_OTHER);
    }
    return rc ? rc : epilogue_x_pass(h, slot, 1, h->psi0);
}

int msl_smatrix_probes(msl_handle* h, const double* xy, int32_t n_probes, int32_t slot) {
    if (!h || !xy) return fail(h, MSL_ERR_INVALID, "msl_smatrix_probes: null argument");
    const msl_config& c = h->cfg;
    if (n_probes != c.n_probes) return fail(h, MSL_ERR_INVALID, "msl_smatrix_probes: %d probes, handle has %d", n_probes, c.n_probes);
    if (!h->sm_built) return fail(h, MSL_ERR_STATE, "msl_smatrix_probes: no S-matrix (msl_smatrix_begin, msl_smatrix_build)");
    if (!h->wf) return fail(h, MSL_ERR_STATE, "msl_smatrix_probes: handle created with n_frames == 0");
    if (slot < 0 || slot >= c.n_frames) return fail(h, MSL_ERR_INVALID, "msl_smatrix_probes: slot %d out of range [0,%d)", slot, c.n_frames);
    for (int k = 0; k < 2 * n_probes; ++k)
        if (!std::isfinite(xy[k])) return fail(h, MSL_ERR_INVALID, "msl_smatrix_probes: position value %d is not finite", k);
    HIPCHK(h, hipSetDevice(c.device));
    int rc;
    if ((rc = h->sm_c.reserve(h, (size_t)h->sm_Bm * n_probes))) return rc;       // (msl_resize_probes keeps S)
    HIPCHK(h, hipMemcpyAsync(h->d_xy, xy, 2 * sizeof(double) * n_probes, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));             // xy is the caller's memory: read before the call returns
    EventPair timer;
    if (c.launch_timing && (rc = timer.begin(h))) return rc;
    if ((rc = begin_timed(h, 8))) return rc;
    if ((rc = smatrix_coefficients(h, n_probes))) return rc;
    // the synthesised waves go to the work buffer (MSL_BUF_EXIT) and to the probe buffer, which the spectrum transform consumes
    h->have_probes = false;
    h->pm_valid = false; h->pm_g = 0;
    const bool vec = c.ny % 2 == 0 && h->pitch % 2 == 0;
    if (n_probes > 8) launch_synth<16>(h, vec, c.nx / h->sm_fx, c.ny / h->sm_fy);
    else launch_synth<8>(h, vec, c.nx / h->sm_fx, c.ny / h->sm_fy);
    HIPCHK(h, hipGetLastError());
    if ((rc = mark_launch(h, K_OTHER))) return rc;
    h->have_exit = true;
    if ((rc = smatrix_spectra(h, n_probes, slot))) return rc;
    h->cur = nullptr;
    const uint64_t img = (uint64_t)c.nx * c.ny * 8ull;
    h->ctr.algorithmic_bytes += (uint64_t)h->sm_Bm * img * (uint64_t)((n_probes + 7) / 8) + (uint64_t)n_probes * (img * 4 + (uint64_t)h->wpix * 8ull);
    return c.launch_timing ? timer.end(h, &h->ctr.ms_propagate) : MSL_OK;
}

extern "C++" template <int G>
static void launch_synth_crop(msl_handle* src, msl_handle* dst, bool vec, int n_probes) {
    const msl_config& c = src->cfg;
    const int lanes_y = vec ? c.ny / 2 : c.ny;
    const dim3 grid((unsigned)((n_probes + G - 1) / G), (unsigned)((c.nx + SM_TILE_ROWS - 1) / SM_TILE_ROWS), (unsigned)((lanes_y + SM_TILE_LANES - 1) / SM_TILE_LANES));
    if (vec) hipLaunchKernelGGL((smatrix_synth_crop_kernel<G, true>), grid, dim3(256), 0, src->stream, (const float2*)src->sm_S.p, (const float2*)src->sm_c.p,
                                (const double*)src->d_xy.p, n_probes, src->sm_Bm, c.nx, c.ny, dst->pitch, dst->cfg.nx, dst->cfg.ny, c.dx, c.dy, dst->psi.p, dst->psi0.p);
    else hipLaunchKernelGGL((smatrix_synth_crop_kernel<G, false>), grid, dim3(256), 0, src->stream, (const float2*)src->sm_S.p, (const float2*)src->sm_c.p,
                            (const double*)src->d_xy.p, n_probes, src->sm_Bm, c.nx, c.ny, dst->pitch, dst->cfg.nx, dst->cfg.ny, c.dx, c.dy, dst->psi.p, dst->psi0.p);
}

int msl_smatrix_probes_cropped(msl_handle* src, msl_handle* dst, const double* xy, int32_t n_probes, int32_t slot) {
    const char* me = "msl_smatrix_probes_cropped";
    if (!src || !dst || !xy) return fail(src ? src : dst, MSL_ERR_INVALID, "%s: null argument", me);
    const msl_config& c = src->cfg;
    const msl_config& d = dst->cfg;
    if (src == dst) return fail(src, MSL_ERR_INVALID, "%s: the source and the result handle are the same", me);
    if (c.device != d.device) return fail(src, MSL_ERR_INVALID, "%s: the handles are on devices %d and %d", me, c.device, d.device);
    if (!src->sm_built) return fail(src, MSL_ERR_STATE, "%s: no S-matrix on the source (msl_smatrix_begin, msl_smatrix_build)", me);
    if (d.nx * src->sm_fx != c.nx || d.ny * src->sm_fy != c.ny)
        return fail(src, MSL_ERR_INVALID, "%s: the result grid %d x %d is not the source's %d x %d divided by its interpolation (%d, %d)", me, d.nx, d.ny,
                    c.nx, c.ny, src->sm_fx, src->sm_fy);
    auto differ = [](double a, double b) { return !(fabs(a - b) <= 1e-12 * fabs(a)); };
    if (differ(c.dx, d.dx) || differ(c.dy, d.dy) || differ(c.wavelength, d.wavelength))
        return fail(src, MSL_ERR_INVALID, "%s: the handles differ in pixel size or wavelength", me);
    if (n_probes != d.n_probes) return fail(src, MSL_ERR_INVALID, "%s: %d probes, the result handle has %d", me, n_probes, d.n_probes);
    if (!dst->wf) return fail(src, MSL_ERR_STATE, "%s: result handle created with n_frames == 0", me);
    if (slot < 0 || slot >= d.n_frames) return fail(src, MSL_ERR_INVALID, "%s: slot %d out of range [0,%d)", me, slot, d.n_frames);
    for (int k = 0; k < 2 * n_probes; ++k)
        if (!std::isfinite(xy[k])) return fail(src, MSL_ERR_INVALID, "%s: position value %d is not finite", me, k);
    HIPCHK(src, hipSetDevice(c.device));
    int rc;
    // the source's probe count only sets the chunk of msl_smatrix_build: c and the positions are held for the result's count
    if ((rc = src->sm_c.reserve(src, (size_t)src->sm_Bm * n_probes)) || (rc = src->d_xy.reserve(src, (size_t)2 * n_probes))) return rc;
    for (auto& e : src->sm_ev)
        if (!e) HIPCHK(src, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    HIPCHK(src, hipMemcpyAsync(src->d_xy, xy, 2 * sizeof(double) * n_probes, hipMemcpyHostToDevice, src->stream));
    HIPCHK(src, hipStreamSynchronize(src->stream));         // xy is the caller's memory: read before the call returns
    EventPair timer;
    if (d.launch_timing && (rc = timer.begin(dst))) return rc;
    if ((rc = begin_timed(src, 4)) || (rc = begin_timed(dst, 4))) return rc;
    if ((rc = smatrix_coefficients(src, n_probes))) return rc;
    // the result handle's earlier work (the reductions of its last batch read the frame slots; its transform the probe buffer) is
    // done before the synthesis, on the source's stream, overwrites its exit and probe buffers
    HIPCHK(src, hipEventRecord(src->sm_ev[0], dst->stream));
    HIPCHK(src, hipStreamWaitEvent(src->stream, src->sm_ev[0], 0));
    dst->have_probes = false;
    dst->pm_valid = false; dst->pm_g = 0;
    // VEC: ny, the cropped ny and the result's work pitch even (the S-matrix is dense: its rows are ny long)
    const bool vec = c.ny % 2 == 0 && d.ny % 2 == 0 && dst->pitch % 2 == 0;
    if (n_probes > 8) launch_synth_crop<16>(src, dst, vec, n_probes);
    else launch_synth_crop<8>(src, dst, vec, n_probes);
    HIPCHK(src, hipGetLastError());
    if ((rc = mark_launch(src, K_OTHER))) return rc;
    src->cur = nullptr;
    // and the synthesis is done before the result handle's transform reads the probe buffer
    HIPCHK(src, hipEventRecord(src->sm_ev[1], src->stream));
    HIPCHK(src, hipStreamWaitEvent(dst->stream, src->sm_ev[1], 0));
    dst->have_exit = true;
    if ((rc = smatrix_spectra(dst, n_probes, slot))) return rc;
    dst->cur = nullptr;
    // S over the windows once per probe group, the folded waves written twice; the transform reads and writes the copy twice and
    // writes the spectra -- all on the cropped image
    const uint64_t img = (uint64_t)d.nx * d.ny * 8ull;
    dst->ctr.algorithmic_bytes += (uint64_t)src->sm_Bm * img * (uint64_t)((n_probes + 7) / 8) + (uint64_t)n_probes * (img * 4 + (uint64_t)dst->wpix * 8ull);
    return d.launch_timing ? timer.end(dst, &dst->ctr.ms_propagate) : MSL_OK;
}

int msl_smatrix_end(msl_handle* h) {
    if (!h) return fail(h, MSL_ERR_INVALID, "msl_smatrix_end: null handle");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    smatrix_release(h);
    return MSL_OK;
}

int msl_tacaw(msl_handle* h, const void* d_src, void* d_dst, int64_t batch, int32_t T, int64_t npix) {
    if (!h) return fail(h, MSL_ERR_INVALID, "null handle");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (!d_src) {
        if (!h->wf) return fail(h, MSL_ERR_STATE, "msl_tacaw: no wavefunction buffer");
        return tacaw_resident(h, h->wf);
    }
    if (!d_dst) return fail(h, MSL_ERR_INVALID, "msl_tacaw: src given without dst");
    return tacaw_run(h, (const float2*)d_src, (float*)d_dst, batch, T, npix);
}

int msl_tacaw_welch_has(int32_t L) { return time_welch_has(L) ? 1 : 0; }

int msl_tacaw_welch(msl_handle* h, const void* d_src, void* d_dst, int64_t batch, int32_t T, int64_t npix, int32_t L, int32_t hop,
                    const double* window_L) {
    if (!h) return fail(h, MSL_ERR_INVALID, "null handle");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (!d_src) {
        if (!h->wf) return fail(h, MSL_ERR_STATE, "msl_tacaw_welch: no wavefunction buffer");
        if (d_dst) return fail(h, MSL_ERR_INVALID, "msl_tacaw_welch: dst given without src");
        return welch_resident(h, h->wf, L, hop, window_L);
    }
    if (!d_dst) return fail(h, MSL_ERR_INVALID, "msl_tacaw_welch: src given without dst");
    int S = 0, rc;
    std::vector<float> g;
    if ((rc = welch_table(h, T, L, hop, window_L, &S, g))) return rc;
    return welch_run(h, (const float2*)d_src, (float*)d_dst, batch, T, npix, L, hop, S, g);
}

int msl_tacaw_stream_begin(msl_handle* h, int32_t T_total, int32_t n_bins, const int32_t* bins) {
    if (!h) return fail(h, MSL_ERR_INVALID, "null handle");
    if (!h->wf) return fail(h, MSL_ERR_STATE, "msl_tacaw_stream_begin: handle created with n_frames == 0 (no frame ring)");
    if (T_total < 2) return fail(h, MSL_ERR_INVALID, "msl_tacaw_stream_begin: needs at least 2 frames (got %d)", T_total);
    if (!bins) n_bins = T_total;
    if (n_bins < 1 || n_bins > T_total) return fail(h, MSL_ERR_INVALID, "msl_tacaw_stream_begin: %d bins of %d", n_bins, T_total);
    std::vector<int> b(n_bins);
    for (int i = 0; i < n_bins; ++i) {
        b[i] = bins ? bins[i] : i;
        if (b[i] < 0 || b[i] >= T_total) return fail(h, MSL_ERR_INVALID, "msl_tacaw_stream_begin: bin %d outside [0,%d)", b[i], T_total);
    }
    const msl_config& c = h->cfg;
    HIPCHK(h, hipSetDevice(c.device));
    const size_t PK = (size_t)c.n_probes * h->wpix;
    int rc;
    if ((rc = h->st_acc.alloc(h, PK * n_bins)) || (rc = h->st_s1.alloc(h, PK)) || (rc = h->st_s2.alloc(h, PK)) ||
        (rc = h->st_tw.alloc(h, (size_t)T_total)) || (rc = h->st_bins.alloc(h, (size_t)n_bins))) return rc;
    std::vector<float2> tw(T_total);
    for (int m = 0; m < T_total; ++m) { const double a = -2.0 * M_PI * m / T_total; tw[m] = make_float2((float)cos(a), (float)sin(a)); }
    HIPCHK(h, hipMemcpyAsync(h->st_tw, tw.data(), tw.size() * sizeof(float2), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->st_bins, b.data(), b.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemsetAsync(h->st_acc, 0, PK * n_bins * sizeof(float2), h->stream));
    HIPCHK(h, hipMemsetAsync(h->st_s1, 0, PK * sizeof(double2), h->stream));
    HIPCHK(h, hipMemsetAsync(h->st_s2, 0, PK * sizeof(double), h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));            // the host vectors go out of scope
    h->st_T = T_total; h->st_F = n_bins; h->st_open = true; h->st_have_ref = false;
    return MSL_OK;
}

int msl_tacaw_stream_set_reference(msl_handle* h, const void* d_ref_c64, int32_t slot) {
    if (!h) return fail(h, MSL_ERR_INVALID, "null handle");
    if (!h->st_open) return fail(h, MSL_ERR_STATE, "msl_tacaw_stream_set_reference: no open stream (msl_tacaw_stream_begin)");
    const msl_config& c = h->cfg;
    if (!d_ref_c64 && (slot < 0 || slot >= c.n_frames))
        return fail(h, MSL_ERR_INVALID, "msl_tacaw_stream_set_reference: slot %d outside the ring of %d", slot, c.n_frames);
    HIPCHK(h, hipSetDevice(c.device));
    const size_t K = h->wpix;
    int rc;
    if (!h->st_ref && (rc = h->st_ref.alloc(h, (size_t)c.n_probes * K))) return rc;
    if (d_ref_c64) {
        HIPCHK(h, hipMemcpyAsync(h->st_ref, d_ref_c64, (size_t)c.n_probes * K * sizeof(float2), hipMemcpyDeviceToDevice, h->stream));
    } else {
        // frame slot `slot` of the (P, ring, K) buffer: P strided images
        HIPCHK(h, hipMemcpy2DAsync(h->st_ref, K * sizeof(float2), h->wf + (size_t)slot * h->wpitch, (size_t)c.n_frames * h->wpitch * sizeof(float2),
                                   K * sizeof(float2), c.n_probes, hipMemcpyDeviceToDevice, h->stream));
    }
    h->st_have_ref = true;
    return MSL_OK;
}

int msl_tacaw_stream_push(msl_handle* h, int32_t first_slot, int32_t count, int32_t t0) {
    if (!h) return fail(h, MSL_ERR_INVALID, "null handle");
    if (!h->st_open) return fail(h, MSL_ERR_STATE, "msl_tacaw_stream_push: no open stream (msl_tacaw_stream_begin)");
    const msl_config& c = h->cfg;
    if (count < 1 || first_slot < 0 || first_slot + count > c.n_frames)
        return fail(h, MSL_ERR_INVALID, "msl_tacaw_stream_push: slots [%d,%d) outside the ring of %d", first_slot, first_slot + count, c.n_frames);
    if (t0 < 0 || t0 + count > h->st_T) return fail(h, MSL_ERR_INVALID, "msl_tacaw_stream_push: times [%d,%d) outside [0,%d)", t0, t0 + count, h->st_T);
    HIPCHK(h, hipSetDevice(c.device));
    FoldJob j{};
    j.wf = h->wf; j.acc = h->st_acc; j.s1 = h->st_s1; j.s2 = h->st_s2; j.tw = h->st_tw; j.bins = h->st_bins;
    j.ref = h->st_have_ref ? h->st_ref.p : nullptr;
    j.K = (long long)h->wpix; j.wfK = (long long)h->wpitch; j.ring = c.n_frames; j.first_slot = first_slot; j.count = count; j.t0 = t0; j.T = h->st_T; j.F = h->st_F;
    const dim3 grid((unsigned)((h->wpix + 255) / 256), c.n_probes);
    for (int f0 = 0; f0 < h->st_F; f0 += MSL_FOLD_FCH) {
        j.f0 = f0;
        hipLaunchKernelGGL(tacaw_fold_kernel, grid, dim3(256), 0, h->stream, j);
    }
    HIPCHK(h, hipGetLastError());
    return MSL_OK;
}

int msl_tacaw_stream_finish_range(msl_handle* h, int32_t p0, int32_t count, void* d_dst_f32, double* total_host) {
    if (!h) return fail(h, MSL_ERR_INVALID, "null handle");
    if (!h->st_open) return fail(h, MSL_ERR_STATE, "msl_tacaw_stream_finish: no open stream");
    const msl_config& c = h->cfg;
    if (p0 < 0 || count < 0 || p0 + count > c.n_probes)
        return fail(h, MSL_ERR_INVALID, "msl_tacaw_stream_finish_range: probes [%d,%d) outside [0,%d)", p0, p0 + count, c.n_probes);
    if (!d_dst_f32 && count > 0 && (p0 != 0 || count != c.n_probes))
        return fail(h, MSL_ERR_INVALID, "msl_tacaw_stream_finish_range: a probe sub-range needs a destination (the handle's intensity buffer holds all probes)");
    HIPCHK(h, hipSetDevice(c.device));
    const size_t PK = (size_t)count * h->wpix, need = PK * h->st_F;
    int rc;
    float* dst = (float*)d_dst_f32;
    if (!dst && count > 0) {
        if (h->intensity.n != need && (rc = h->intensity.alloc(h, need))) return rc;
        h->intensity_F = h->st_F; h->intensity_ld = h->wpix;
        dst = h->intensity;
    }
    if (need) {
        hipLaunchKernelGGL(tacaw_stream_finish_kernel, dim3((unsigned)((need + 255) / 256)), dim3(256), 0, h->stream,
                           h->st_acc + (size_t)p0 * h->st_F * h->wpix, dst, h->st_bins, (long long)h->st_F, (long long)h->wpix, (long long)need);
        HIPCHK(h, hipGetLastError());
    }
    if (total_host && PK) {
        if ((rc = h->scratch.reserve(h, PK * sizeof(double)))) return rc;
        hipLaunchKernelGGL(tacaw_stream_total_kernel, dim3((unsigned)((PK + 255) / 256)), dim3(256), 0, h->stream, h->st_s1 + (size_t)p0 * h->wpix,
                           h->st_s2 + (size_t)p0 * h->wpix, (double)h->st_T, (long long)PK, (double*)h->scratch.p);
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipMemcpyAsync(total_host, h->scratch, PK * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->st_acc.release();                                    // the accumulators are the big part: give them back
    h->st_open = false;
    return MSL_OK;
}

int msl_tacaw_stream_finish(msl_handle* h, double* total_PK) {
    if (!h) return fail(h, MSL_ERR_INVALID, "null handle");
    return msl_tacaw_stream_finish_range(h, 0, h->cfg.n_probes, nullptr, total_PK);
}

size_t msl_buffer_bytes(const msl_handle* h, msl_buffer what) {
    if (!h) return 0;
    const msl_config& c = h->cfg;
    const size_t npix = (size_t)c.nx * c.ny;
    switch (what) {
        case MSL_BUF_PROBES: case MSL_BUF_EXIT: return npix * c.n_probes * 8;
        case MSL_BUF_POTENTIAL: return (h->V || h->abs_built) ? npix * c.nz * 4 : 0;
        case MSL_BUF_TRANSMISSION: return npix * c.nz * 8;
        case MSL_BUF_WAVEFUNCTION: return h->wf ? h->wpitch * c.n_probes * c.n_frames * 8 : 0;
        case MSL_BUF_INTENSITY: return h->intensity.n * 4;
        case MSL_BUF_FORMFACTOR: return h->fin_nch ? 0 : npix * h->n_species * 4;      // (under finite projection d_ff holds the channel tables)
        case MSL_BUF_FORMFACTOR_FINITE: return (h->fin_nch && h->ff_n > 0) ? npix * (size_t)h->fin_nch * 4 : 0;
        case MSL_BUF_STREAM_ACC: return (h->st_open && h->st_acc) ? h->wpix * c.n_probes * (size_t)h->st_F * 8 : 0;
        case MSL_BUF_STREAM_S1: return (h->st_open && h->st_s1) ? h->wpix * c.n_probes * 16 : 0;
        case MSL_BUF_STREAM_S2: return (h->st_open && h->st_s2) ? h->wpix * c.n_probes * 8 : 0;
        case MSL_BUF_STREAM_REF: return (h->st_open && h->st_have_ref) ? h->wpix * c.n_probes * 8 : 0;
        case MSL_BUF_LAYERS: return h->wf ? n_result_layers(h) * layer_block_elems(h) * 8 : 0;
        case MSL_BUF_SMATRIX: return h->sm_built ? npix * (size_t)h->sm_Bm * 8 : 0;
        case MSL_BUF_FORMFACTOR_ABS: return (h->abs_on && h->abs_absorb && h->d_ffa && h->ff_n > 0) ? npix * h->n_species * 4 : 0;
        case MSL_BUF_ABSORPTION: return (h->abs_built && h->abs_absorb && h->abs_O) ? npix * c.nz * 4 : 0;
        case MSL_BUF_FORMFACTOR_TDS: return (h->tds_on && h->tds_g && h->ff_n > 0) ? npix * h->n_species * h->tds_n * 4 : 0;
        case MSL_BUF_TDS_WEIGHT: return (h->tds_on && h->abs_built && h->tds_W) ? npix * c.nz * h->tds_n * 4 : 0;
        case MSL_BUF_IONIZATION_WEIGHT: return (h->ion_on && h->ion_built && h->ion_W) ? npix * c.nz * h->ion_n * 4 : 0;
    }
    return 0;
}

int64_t msl_result_pitch(const msl_handle* h, msl_buffer what) {
    if (!h) return 0;
    if (what == MSL_BUF_WAVEFUNCTION || what == MSL_BUF_LAYERS) return h->wf ? (int64_t)h->wpitch : 0;
    if (what == MSL_BUF_INTENSITY) return h->intensity ? (int64_t)h->intensity_ld : 0;
    return 0;
}

void* msl_device_ptr(msl_handle* h, msl_buffer what) {
    if (!h) return nullptr;
    switch (what) {
        case MSL_BUF_PROBES: return h->psi0;
        case MSL_BUF_EXIT: return h->psi;
        case MSL_BUF_POTENTIAL: return h->abs_built ? h->abs_V + (size_t)h->cur_batch * h->cfg.nz * h->cfg.nx * h->cfg.ny : h->V.p;     // Vbar of the current stack
        case MSL_BUF_TRANSMISSION: return h->trans ? h->trans + (size_t)h->cur_batch * h->cfg.nz * h->cfg.nx * h->cfg.ny : nullptr;
        case MSL_BUF_WAVEFUNCTION: return h->wf;
        case MSL_BUF_INTENSITY: return h->intensity;
        case MSL_BUF_FORMFACTOR: return h->d_ff;
        case MSL_BUF_FORMFACTOR_FINITE: return h->fin_nch ? h->d_ff.p : nullptr;
        case MSL_BUF_STREAM_ACC: return h->st_open ? h->st_acc.p : nullptr;
        case MSL_BUF_STREAM_S1: return h->st_open ? h->st_s1.p : nullptr;
        case MSL_BUF_STREAM_S2: return h->st_open ? h->st_s2.p : nullptr;
        case MSL_BUF_STREAM_REF: return (h->st_open && h->st_have_ref) ? h->st_ref.p : nullptr;
        case MSL_BUF_LAYERS: return h->layers;
        case MSL_BUF_SMATRIX: return h->sm_S;
        case MSL_BUF_FORMFACTOR_ABS: return h->d_ffa;
        case MSL_BUF_ABSORPTION: return h->abs_O ? h->abs_O + (size_t)h->cur_batch * h->cfg.nz * h->cfg.nx * h->cfg.ny : nullptr;
        case MSL_BUF_FORMFACTOR_TDS: return h->tds_g;
        case MSL_BUF_TDS_WEIGHT: return h->tds_W;
        case MSL_BUF_IONIZATION_WEIGHT: return h->ion_W;
    }
    return nullptr;
}

// ---- reductions over resident results (reduce.h) ------------------------------------------------------
// The rows a reduction reads: (B, R, K) elements at p, R the frame or frequency axis, rows ld elements apart.
struct Rows { const void* p; int64_t B, R, K, ld; };

// what a NULL source means, and what else resolve_rows() refuses
enum : unsigned {
    SRC_INTENSITY = 0,         // NULL = the handle's intensity buffer (after msl_tacaw)
    SRC_WAVEFUNCTION = 1,      // NULL = the exit block of the handle's resident result
    SRC_FIRST_B = 2,           // NULL reads the first B probes (B < 1: every probe); without it, always every probe
    SRC_INT32_ROWS = 4,        // B * R must fit 31 bits
};

// The one source convention of every reduction: r holds the caller's (src, B, R, K, ld).  src = NULL asks for the resident
// buffer that `flags` names, with its own R, K and pitch; a pointer with ld = 0 has rows of pitch K.
static int resolve_rows(msl_handle* h, const char* who, unsigned flags, Rows* r) {
    if (!h) return fail(h, MSL_ERR_INVALID, "null handle");
    if (!r->p) {
        const bool wf = flags & SRC_WAVEFUNCTION;
        if (!(wf ? (const void*)h->wf : (const void*)h->intensity.p))
            return fail(h, MSL_ERR_STATE, wf ? "%s: no wavefunction buffer" : "%s: no intensity (call msl_tacaw)", who);
        if (!(flags & SRC_FIRST_B) || r->B < 1) r->B = h->cfg.n_probes;
        if (r->B > h->cfg.n_probes) return fail(h, MSL_ERR_INVALID, "%s: %lld probes, the handle has %d", who, (long long)r->B, h->cfg.n_probes);
        if (wf) *r = Rows{h->wf, r->B, h->cfg.n_frames, (int64_t)h->wpix, (int64_t)h->wpitch};
        else *r = Rows{h->intensity.p, r->B, h->intensity_F, (int64_t)h->wpix, (int64_t)h->intensity_ld};
    } else if (r->ld == 0) {
        r->ld = r->K;
    }
    if (r->B < 1 || r->R < 1 || r->K < 1) return fail(h, MSL_ERR_INVALID, "%s: bad shape (%lld,%lld,%lld)", who, (long long)r->B, (long long)r->R, (long long)r->K);
    if (r->ld < r->K) return fail(h, MSL_ERR_INVALID, "%s: row pitch %lld below the row length %lld", who, (long long)r->ld, (long long)r->K);
    if ((flags & SRC_INT32_ROWS) && r->B * r->R > 0x7fffffffLL) return fail(h, MSL_ERR_UNSUPPORTED, "%s: more than 2^31 rows", who);
    return MSL_OK;
}

// rows [t0, t0 + count) of an axis of n `what` ("frame slots", "frequency bins")
static int check_slots(msl_handle* h, const char* who, const char* what, int64_t t0, int64_t count, int64_t n) {
    if (count < 1 || t0 < 0 || t0 + count > n)
        return fail(h, MSL_ERR_INVALID, "%s: %s [%lld,%lld) outside [0,%lld)", who, what, (long long)t0, (long long)(t0 + count), (long long)n);
    return MSL_OK;
}

// a bx x by bin that divides a wx x wy window
static int check_window_bin(msl_handle* h, const char* who, int wx, int wy, int bx, int by) {
    if (wx < 1 || wy < 1) return fail(h, MSL_ERR_INVALID, "%s: window %d x %d", who, wx, wy);
    if (bx < 1 || by < 1 || wx % bx || wy % by) return fail(h, MSL_ERR_INVALID, "%s: bin %d x %d does not divide the window %d x %d", who, bx, by, wx, wy);
    return MSL_OK;
}

// device to host on the handle's stream, and wait for it
static int download_sync(msl_handle* h, void* dst, const void* src, size_t bytes) {
    HIPCHK(h, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return MSL_OK;
}

// out[r] = the sum of the n_chunks partial sums of row r
static void sum_row_parts(const std::vector<double>& part, int64_t rows, int n_chunks, double* out) {
    for (int64_t r = 0; r < rows; ++r) {
        double s = 0;
        for (int c = 0; c < n_chunks; ++c) s += part[(size_t)r * n_chunks + c];
        out[r] = s;
    }
}

// sum over K of rows of a (rows, K) array (row pitch ld) with an optional host mask; float64 result per row on the host
static int reduce_rows(msl_handle* h, const void* src, bool complex_abs, int64_t rows, int64_t K, int64_t ld, const uint8_t* mask, double* out) {
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const int64_t quads = (K + 3) / 4;
    int n_chunks = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(quads / 1024, 4096 / rows), 64));
    const size_t mask_bytes = mask ? (((size_t)K + 15) & ~(size_t)15) + 16 : 0;
    const size_t part_bytes = (size_t)rows * n_chunks * sizeof(double);
    int rc = h->scratch.reserve(h, mask_bytes + part_bytes);
    if (rc) return rc;
    uint8_t* d_mask = mask ? (uint8_t*)h->scratch.p : nullptr;
    double* d_part = (double*)(h->scratch + mask_bytes);
    if (mask) {
        HIPCHK(h, hipMemsetAsync(d_mask, 0, mask_bytes, h->stream));
        HIPCHK(h, hipMemcpyAsync(d_mask, mask, (size_t)K, hipMemcpyHostToDevice, h->stream));
    }
    with_bool(complex_abs, [&](auto c_abs) {
        hipLaunchKernelGGL(reduce_k_kernel<decltype(c_abs)::value>, dim3(n_chunks, (unsigned)rows), dim3(256), 0, h->stream, src, d_mask, (long long)K,
                           (long long)ld, n_chunks, d_part);
    });
    HIPCHK(h, hipGetLastError());
    std::vector<double> part((size_t)rows * n_chunks);
    if ((rc = download_sync(h, part.data(), d_part, part_bytes))) return rc;
    sum_row_parts(part, rows, n_chunks, out);
    return MSL_OK;
}

int msl_tacaw_spectrum(msl_handle* h, const void* d_src_f32, int64_t B, int64_t F, int64_t K, int64_t ld, const uint8_t* mask, double* out) {
    if (!out) return fail(h, MSL_ERR_INVALID, "msl_tacaw_spectrum: null output");
    Rows r{d_src_f32, B, F, K, ld};
    int rc = resolve_rows(h, "msl_tacaw_spectrum", SRC_INTENSITY | SRC_INT32_ROWS, &r);
    if (rc) return rc;
    if (r.B * r.R > 65535) {                   // grid.y limit: go probe by probe
        if (r.R > 65535) return fail(h, MSL_ERR_UNSUPPORTED, "msl_tacaw_spectrum: more than 65535 frequencies");
        for (int64_t b = 0; b < r.B; ++b)
            if ((rc = reduce_rows(h, (const float*)r.p + b * r.R * r.ld, false, r.R, r.K, r.ld, mask, out + b * r.R))) return rc;
        return MSL_OK;
    }
    return reduce_rows(h, r.p, false, r.B * r.R, r.K, r.ld, mask, out);
}

int msl_tacaw_spectrum_weighted(msl_handle* h, const void* d_src_f32, int64_t B, int64_t F, int64_t K, int64_t ld, const double* weight, double* out) {
    if (!out || !weight) return fail(h, MSL_ERR_INVALID, "msl_tacaw_spectrum_weighted: null argument");
    Rows r{d_src_f32, B, F, K, ld};
    int rc = resolve_rows(h, "msl_tacaw_spectrum_weighted", SRC_INTENSITY | SRC_INT32_ROWS, &r);
    if (rc) return rc;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const int64_t all = r.B * r.R, rows_per = std::min<int64_t>(all, 32768);
    const int n_chunks = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(r.K / 4096, 4096 / std::max<int64_t>(1, rows_per)), 64));
    const size_t w_bytes = (size_t)r.K * sizeof(double), part_bytes = (size_t)rows_per * n_chunks * sizeof(double);
    if ((rc = h->scratch.reserve(h, w_bytes + part_bytes))) return rc;
    double* d_w = (double*)h->scratch.p;
    double* d_part = (double*)(h->scratch + w_bytes);
    HIPCHK(h, hipMemcpyAsync(d_w, weight, w_bytes, hipMemcpyHostToDevice, h->stream));
    std::vector<double> part((size_t)rows_per * n_chunks);
    for (int64_t r0 = 0; r0 < all; r0 += rows_per) {
        const int64_t rows = std::min<int64_t>(rows_per, all - r0);
        hipLaunchKernelGGL(reduce_kw_kernel, dim3(n_chunks, (unsigned)rows), dim3(256), 0, h->stream, (const float*)r.p + r0 * r.ld, d_w,
                           (long long)r.K, (long long)r.ld, n_chunks, d_part);
        HIPCHK(h, hipGetLastError());
        if ((rc = download_sync(h, part.data(), d_part, (size_t)rows * n_chunks * sizeof(double)))) return rc;
        sum_row_parts(part, rows, n_chunks, out + r0);
    }
    return MSL_OK;
}

int msl_adf(msl_handle* h, const void* d_src_c64, int64_t B, int64_t T, int64_t K, int64_t ld, const uint8_t* mask, double* out) {
    if (!h || !out) return fail(h, MSL_ERR_INVALID, "msl_adf: null argument");
    Rows r{d_src_c64, B, T, K, ld};
    int rc = resolve_rows(h, "msl_adf", SRC_WAVEFUNCTION, &r);              // the resident result: always every probe
    if (rc) return rc;
    if (r.R > 65535) return fail(h, MSL_ERR_UNSUPPORTED, "msl_adf: more than 65535 frames");
    std::vector<double> rows((size_t)r.R);
    for (int64_t b = 0; b < r.B; ++b) {
        if ((rc = reduce_rows(h, (const float2*)r.p + b * r.R * r.ld, true, r.R, r.K, r.ld, mask, rows.data()))) return rc;
        double s = 0;
        for (double v : rows) s += v;
        out[b] = s / (double)r.R;              // mean over frames of the annulus sum (haadf_data.py:80)
    }
    return MSL_OK;
}

// ---- STEM detectors (detect.h) ----------------------------------------------------------------------------
int msl_set_detectors(msl_handle* h, int32_t n, const uint16_t* member_K, const int32_t* signal_n, const float* kx_wx, const float* ky_wy) {
    if (!h || !member_K || !signal_n || !kx_wx || !ky_wy) return fail(h, MSL_ERR_INVALID, "msl_set_detectors: null argument");
    if (n < 1 || n > DET_MAX) return fail(h, MSL_ERR_INVALID, "msl_set_detectors: %d detectors outside [1,%d]", n, DET_MAX);
    // the staging of the layer reductions has rows of the detector count it was set up with: other masks are fine, another count is not
    if (h->lr_on && (h->lr_what & LR_DETECT) && n != (int)h->lr_lay.D)
        return fail(h, MSL_ERR_STATE, "msl_set_detectors: %d detectors while the layer reductions are set up for %d (clear msl_set_layer_reduce first)",
                    n, (int)h->lr_lay.D);
    uint32_t amp = 0, cx = 0, cy = 0;
    for (int d = 0; d < n; ++d) {
        switch (signal_n[d]) {
            case MSL_DET_INTENSITY: break;
            case MSL_DET_AMPLITUDE: amp |= 1u << d; break;
            case MSL_DET_COM_X: cx |= 1u << d; break;
            case MSL_DET_COM_Y: cy |= 1u << d; break;
            default: return fail(h, MSL_ERR_INVALID, "msl_set_detectors: detector %d has unknown signal %d", d, signal_n[d]);
        }
    }
    const int sx = h->wx / h->bx, sy = h->wy / h->by;         // stored k axes: the (binned) window
    const size_t K = h->wpix;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    std::vector<uint16_t> m(member_K, member_K + K);
    const uint16_t keep = (uint16_t)((1u << n) - 1u);
    for (auto& v : m) v &= keep;                               // bits of absent detectors never count
    int rc;
    if ((rc = h->det_mask.alloc(h, K)) || (rc = h->det_kx.alloc(h, (size_t)sx)) || (rc = h->det_ky.alloc(h, (size_t)sy))) {
        h->det_n = 0;
        return rc;
    }
    HIPCHK(h, hipMemcpyAsync(h->det_mask, m.data(), K * sizeof(uint16_t), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->det_kx, kx_wx, (size_t)sx * sizeof(float), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->det_ky, ky_wy, (size_t)sy * sizeof(float), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->det_n = n; h->det_K = K; h->det_wy = sy;
    h->det_amp = amp; h->det_cx = cx; h->det_cy = cy;
    return MSL_OK;
}

// The tiling of a detector pass (detect.h) over `rows` rows of K pixels with n detectors: every workgroup of the tile kernel
// writes ND partial sums per row and tile to d_part, detect_finish_kernel<ND> adds them to the (rows, n) float64 at d_out.
struct DetTiling {
    int n, ND;                                  // detectors, and their padded count: 4, 8 or 16
    int64_t rows, n_tiles, per, blocks_y;       // tiles of 64 * (64 / ND) pixels along a row; rows per workgroup; grid.y
    size_t part_bytes, out_bytes;
    float* d_part;
    double* d_out;
    dim3 grid() const { return dim3((unsigned)n_tiles, (unsigned)blocks_y); }
};

// the arithmetic of it, which needs no device
static DetTiling det_tiling(int64_t rows, int64_t K, int n) {
    DetTiling t{};
    t.n = n; t.rows = rows;
    t.ND = n <= 4 ? 4 : (n <= 8 ? 8 : 16);
    const int64_t TP = 64 * (64 / t.ND);
    t.n_tiles = (K + TP - 1) / TP;
    // rows per workgroup: the tile's coefficients are built once per row block; at most 65535 row blocks (grid.y)
    t.per = std::min<int64_t>(64, (rows + 3) / 4 * 4);
    t.per = std::max<int64_t>(t.per, ((rows + 65534) / 65535 + 3) / 4 * 4);
    t.blocks_y = (rows + t.per - 1) / t.per;
    t.part_bytes = ((size_t)rows * t.n_tiles * t.ND * sizeof(float) + 255) & ~(size_t)255;
    t.out_bytes = (size_t)rows * n * sizeof(double);
    return t;
}

// the preconditions that msl_detect and msl_spectrum_detect share, then the tiling of the `count` rows per probe from t0 on,
// with its two pieces of h->scratch; d_dst: a device destination of the (rows, n) result instead of the second piece
static int plan_detect(msl_handle* h, const char* who, const Rows& r, const char* what, int32_t t0, int32_t count, DetTiling* t,
                       double* d_dst = nullptr) {
    if ((size_t)r.K != h->det_K) return fail(h, MSL_ERR_INVALID, "%s: rows of %lld pixels, the detectors cover %zu", who, (long long)r.K, h->det_K);
    int rc = check_slots(h, who, what, t0, count, r.R);
    if (rc) return rc;
    if (r.B * count > 0x7fffffffLL) return fail(h, MSL_ERR_UNSUPPORTED, "%s: more than 2^31 rows", who);
    *t = det_tiling(r.B * count, r.K, h->det_n);
    if (t->n_tiles > 0x7fffffffLL) return fail(h, MSL_ERR_UNSUPPORTED, "%s: rows too long", who);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if ((rc = h->scratch.reserve(h, t->part_bytes + (d_dst ? 0 : t->out_bytes)))) return rc;
    t->d_part = (float*)h->scratch.p;
    t->d_out = d_dst ? d_dst : (double*)(h->scratch + t->part_bytes);
    return MSL_OK;
}

// the tile kernel of msl_detect over the planned rows, queued
static int detect_tiles(msl_handle* h, const Rows& r, int32_t t0, int32_t count, const DetTiling& t) {
    const int mode = h->det_amp == 0 ? 0 : (h->det_amp == (1u << t.n) - 1u ? 1 : 2);
    const bool vec = (r.ld % 2 == 0) && (((uintptr_t)r.p & 15) == 0);
    with_int<4, 8, 16>(t.ND, [&](auto nd) { with_int<0, 1, 2>(mode, [&](auto m) { with_bool(vec, [&](auto v) {
        hipLaunchKernelGGL((detect_tile_kernel<decltype(nd)::value, decltype(m)::value, decltype(v)::value>), t.grid(), dim3(256), 0, h->stream,
                           (const float2*)r.p, (long long)r.R, (long long)t0, (long long)count, (long long)r.ld, (long long)r.K, (long long)t.rows, (int)t.per,
                           h->det_mask.p, h->det_kx.p, h->det_ky.p, h->det_wy, h->det_amp, h->det_cx, h->det_cy, t.d_part);
    }); }); });
    HIPCHK(h, hipGetLastError());
    return MSL_OK;
}

// after the tile kernel: the sums over the tiles into t.d_out, queued
static int detect_finish(msl_handle* h, const DetTiling& t) {
    HIPCHK(h, hipGetLastError());
    with_int<4, 8, 16>(t.ND, [&](auto nd) {
        hipLaunchKernelGGL(detect_finish_kernel<decltype(nd)::value>, dim3((unsigned)t.rows), dim3(256), 0, h->stream, t.d_part, (long long)t.n_tiles, t.n,
                           t.d_out);
    });
    HIPCHK(h, hipGetLastError());
    return MSL_OK;
}

int msl_detect(msl_handle* h, const void* d_src_c64, int64_t B, int64_t T, int64_t K, int64_t ld, int32_t t0, int32_t count, double* out) {
    if (!h || !out) return fail(h, MSL_ERR_INVALID, "msl_detect: null argument");
    if (h->det_n == 0) return fail(h, MSL_ERR_STATE, "msl_detect: no detectors (call msl_set_detectors)");
    Rows r{d_src_c64, B, T, K, ld};
    DetTiling t;
    int rc;
    if ((rc = resolve_rows(h, "msl_detect", SRC_WAVEFUNCTION | SRC_FIRST_B, &r)) || (rc = plan_detect(h, "msl_detect", r, "frame slots", t0, count, &t)) ||
        (rc = detect_tiles(h, r, t0, count, t)) || (rc = detect_finish(h, t))) return rc;
    return download_sync(h, out, t.d_out, t.out_bytes);
}

// ---- polar detector (polar.h) -----------------------------------------------------------------------------
static int check_polar_map(msl_handle* h, const char* who, const uint16_t* bin_K, int64_t K, int32_t n_bins) {
    if (!bin_K) return fail(h, MSL_ERR_INVALID, "%s: null argument", who);
    if (K < 0) return fail(h, MSL_ERR_INVALID, "%s: %lld pixels", who, (long long)K);
    if (n_bins < 1 || n_bins > POLAR_MAX_BINS) return fail(h, MSL_ERR_INVALID, "%s: %d bins outside [1,%d]", who, n_bins, POLAR_MAX_BINS);
    return MSL_OK;
}

int msl_polar_layout(const uint16_t* bin_K, int64_t K, int32_t n_bins, uint32_t* order_K, int64_t* seg_n1) {
    int rc = check_polar_map(nullptr, "msl_polar_layout", bin_K, K, n_bins);
    if (rc) return rc;
    if (!order_K || !seg_n1) return fail(nullptr, MSL_ERR_INVALID, "msl_polar_layout: null argument");
    if (!polar_layout(bin_K, K, n_bins, order_K, seg_n1))
        return fail(nullptr, MSL_ERR_INVALID, "msl_polar_layout: a bin id outside [0,%d) that is not MSL_POLAR_NONE", n_bins);
    return MSL_OK;
}

int msl_set_polar(msl_handle* h, int32_t n_bins, const uint16_t* bin_K) {
    if (!h) return fail(h, MSL_ERR_INVALID, "msl_set_polar: null handle");
    const size_t K = h->wpix;
    int rc = check_polar_map(h, "msl_set_polar", bin_K, (int64_t)K, n_bins);
    if (rc) return rc;
    if (K > 0xffffffffull) return fail(h, MSL_ERR_UNSUPPORTED, "msl_set_polar: more than 2^32 stored pixels");
    if (h->lr_on && (h->lr_what & LR_POLAR) && n_bins != (int)h->lr_lay.n_bins)     // (as msl_set_detectors: the staging has rows of n_bins)
        return fail(h, MSL_ERR_STATE, "msl_set_polar: %d bins while the layer reductions are set up for %d (clear msl_set_layer_reduce first)", n_bins,
                    (int)h->lr_lay.n_bins);
    h->pol_bins = 0;
    std::vector<uint32_t> order(std::max<size_t>(K, 1));
    std::vector<int64_t> seg((size_t)n_bins + 1);
    if (!polar_layout(bin_K, (int64_t)K, n_bins, order.data(), seg.data()))
        return fail(h, MSL_ERR_INVALID, "msl_set_polar: a bin id outside [0,%d) that is not MSL_POLAR_NONE", n_bins);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if ((rc = h->pol_order.alloc(h, order.size())) || (rc = h->pol_seg.alloc(h, seg.size()))) return rc;
    HIPCHK(h, hipMemcpyAsync(h->pol_order, order.data(), order.size() * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->pol_seg, seg.data(), seg.size() * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->pol_bins = n_bins; h->pol_K = K;
    return MSL_OK;
}

// the gather of msl_polar_detect over resolved rows, queued: the (rows, n_bins) float64 result goes to d_dst, or with d_dst == NULL
// to h->scratch; *d_res / *res_bytes name it
static int polar_launch(msl_handle* h, const Rows& r, int32_t t0, int32_t count, double* d_dst, double** d_res, size_t* res_bytes) {
    int rc;
    if ((size_t)r.K != h->pol_K) return fail(h, MSL_ERR_INVALID, "msl_polar_detect: rows of %lld pixels, the bin map covers %zu", (long long)r.K, h->pol_K);
    if ((rc = check_slots(h, "msl_polar_detect", "frame slots", t0, count, r.R))) return rc;
    const int64_t rows = r.B * count, n_bins = h->pol_bins;
    if (rows > 0x7fffffffLL) return fail(h, MSL_ERR_UNSUPPORTED, "msl_polar_detect: more than 2^31 rows");
    // rows per workgroup: a wave reads its bin's pixel list once per POLAR_ROWS rows; whole groups of them while that leaves about
    // 64 k waves to spread over the device, and as many as the grid's 2^31 workgroups need
    const int64_t bin_groups = (n_bins + POLAR_WAVES - 1) / POLAR_WAVES;
    int64_t per = std::max<int64_t>(1, std::min<int64_t>(16, rows * n_bins / 65536 / POLAR_ROWS)) * POLAR_ROWS;
    per = std::max<int64_t>(per, ((rows * bin_groups + 0x7ffffffeLL) / 0x7fffffffLL + POLAR_ROWS - 1) / POLAR_ROWS * POLAR_ROWS);
    const int64_t row_blocks = (rows + per - 1) / per;
    const size_t out_bytes = (size_t)rows * n_bins * sizeof(double);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (!d_dst && (rc = h->scratch.reserve(h, out_bytes))) return rc;
    double* d_out = d_dst ? d_dst : (double*)h->scratch.p;
    hipLaunchKernelGGL(polar_gather_kernel, dim3((unsigned)(row_blocks * bin_groups)), dim3(64 * POLAR_WAVES), 0, h->stream, (const float2*)r.p,
                       (long long)r.R, (long long)t0, (unsigned)count, (long long)r.ld, (long long)rows, (int)per, (int)n_bins, (unsigned)bin_groups,
                       h->pol_order.p, h->pol_seg.p, d_out);
    HIPCHK(h, hipGetLastError());
    *d_res = d_out; *res_bytes = out_bytes;
    return MSL_OK;
}

int msl_polar_detect(msl_handle* h, const void* d_src_c64, int64_t B, int64_t T, int64_t K, int64_t ld, int32_t t0, int32_t count, double* out) {
    if (!h || !out) return fail(h, MSL_ERR_INVALID, "msl_polar_detect: null argument");
    if (h->pol_bins == 0) return fail(h, MSL_ERR_STATE, "msl_polar_detect: no bin map (call msl_set_polar)");
    Rows r{d_src_c64, B, T, K, ld};
    int rc;
    double* d_out = nullptr;
    size_t out_bytes = 0;
    if ((rc = resolve_rows(h, "msl_polar_detect", SRC_WAVEFUNCTION | SRC_FIRST_B, &r)) || (rc = polar_launch(h, r, t0, count, nullptr, &d_out, &out_bytes))) return rc;
    return download_sync(h, out, d_out, out_bytes);
}

// ---- spectrum detectors (spectrum_detect.h) ---------------------------------------------------------------
int msl_spectrum_detect(msl_handle* h, const void* d_src_f32, int64_t B, int64_t F, int64_t K, int64_t ld, int32_t f0, int32_t count, double* out) {
    if (!h || !out) return fail(h, MSL_ERR_INVALID, "msl_spectrum_detect: null argument");
    if (h->det_n == 0) return fail(h, MSL_ERR_STATE, "msl_spectrum_detect: no detectors (call msl_set_detectors)");
    if (h->det_amp | h->det_cx | h->det_cy)
        return fail(h, MSL_ERR_INVALID, "msl_spectrum_detect: every detector must have the intensity signal (an amplitude or centre-of-mass "
                                        "weight of a TACAW intensity is not defined)");
    Rows r{d_src_f32, B, F, K, ld};
    DetTiling t;
    int rc;
    if ((rc = resolve_rows(h, "msl_spectrum_detect", SRC_INTENSITY | SRC_FIRST_B, &r)) ||
        (rc = plan_detect(h, "msl_spectrum_detect", r, "frequency bins", f0, count, &t))) return rc;
    // pixels per load: the rows start at src + row * ld floats, the tiles at multiples of 256 pixels
    const uintptr_t base = (uintptr_t)r.p;
    const int vw = (r.ld % 4 == 0 && (base & 15) == 0) ? 4 : ((r.ld % 2 == 0 && (base & 7) == 0) ? 2 : 1);
    with_int<4, 8, 16>(t.ND, [&](auto nd) { with_int<4, 2, 1>(vw, [&](auto w) {
        hipLaunchKernelGGL((spectrum_tile_kernel<decltype(nd)::value, decltype(w)::value>), t.grid(), dim3(256), 0, h->stream, (const float*)r.p,
                           (long long)r.R, (long long)f0, (long long)count, (long long)r.ld, (long long)r.K, (long long)t.rows, (int)t.per, h->det_mask.p,
                           t.d_part);
    }); });
    if ((rc = detect_finish(h, t))) return rc;
    return download_sync(h, out, t.d_out, t.out_bytes);
}

// ---- diffraction patterns (diffract.h) --------------------------------------------------------------------
// What the pattern pass of msl_diffract and of msl_diffract_members share, checked and computed in one place: the window, the bin
// and the frame slots against the rows, then the bin mode, the load width and the launch shape for `waves_per_strip` waves of the source
// per strip (1: a strip is a row of bins of one probe; G: of one position, ensemble.h) and `lds_totals` more doubles of LDS per bin of a
// strip in the LDS mode.
struct DiffractPlan {
    int mx, my, mode;
    bool vec;
    int64_t strips, per;
    size_t lds, n_out;
    unsigned threads, grid;
};

static int plan_diffract(msl_handle* h, const char* who, const Rows& r, int32_t t0, int32_t count, int32_t wx, int32_t wy, int32_t bx, int32_t by,
                         int waves_per_strip, int lds_totals, DiffractPlan* p) {
    int rc;
    if ((rc = check_window_bin(h, who, wx, wy, bx, by))) return rc;
    if ((int64_t)wx * wy != r.K) return fail(h, MSL_ERR_INVALID, "%s: window %d x %d over rows of %lld pixels", who, wx, wy, (long long)r.K);
    if ((rc = check_slots(h, who, "frame slots", t0, count, r.R))) return rc;
    p->mx = wx / bx; p->my = wy / by;
    p->strips = r.B / waves_per_strip * p->mx;
    if ((int64_t)count * bx > 0x3fffffffLL) return fail(h, MSL_ERR_UNSUPPORTED, "%s: more than 2^30 rows per bin", who);
    const bool pow2 = (by & (by - 1)) == 0;
    p->mode = by == 1 ? DIFF_DIRECT : (pow2 && by <= 64 ? DIFF_SHFL : DIFF_LDS);
    p->lds = p->mode == DIFF_LDS ? ((size_t)wy + (size_t)lds_totals * p->my) * sizeof(double) : 0;
    if (p->lds > 64u * 1024u) return fail(h, MSL_ERR_UNSUPPORTED, "%s: bin %d of rows of %d pixels needs %zu bytes of LDS", who, by, wy, p->lds);
    p->n_out = (size_t)p->strips * p->my;
    // 16-byte loads need every row to start on 16 bytes: base, image pitch and row length even in pixels
    p->vec = (r.ld % 2 == 0) && (wy % 2 == 0) && (((uintptr_t)r.p & 15) == 0);
    const int cols = p->vec ? (wy + 1) / 2 : wy;
    p->threads = (unsigned)std::min(256, std::max(64, (cols + 63) / 64 * 64));
    // strips per workgroup: about 64 KB of reads each, but at least 4096 workgroups while there are that many strips
    const int64_t strip_bytes = (int64_t)waves_per_strip * count * bx * wy * 8;
    int64_t per = std::max<int64_t>(1, 65536 / strip_bytes);
    per = std::max<int64_t>(1, std::min<int64_t>(per, p->strips / 4096));
    p->per = std::max<int64_t>(per, (p->strips + 0x7ffffffeLL) / 0x7fffffffLL);
    p->grid = (unsigned)((p->strips + p->per - 1) / p->per);
    return MSL_OK;
}

// the G member waves per position and their weights of a members call (ensemble.h); a null pointer to it: the plain call
struct Members {
    int32_t G;
    const double* weights;
};

// the pattern pass over resolved rows, queued as one timed launch: msl_diffract's (B, mx, my) float64 result, or with `m` the
// (B / G, mx, my) member totals of msl_diffract_members.  It is added to d_acc (the dose accumulator) where that is given, else stored
// to d_dst, else to h->diff_out; *d_res / *res_bytes name it.
static int pattern_launch(msl_handle* h, const char* who, const Rows& r, int32_t t0, int32_t count, int32_t wx, int32_t wy, int32_t bx, int32_t by,
                          const Members* m, double* d_dst, double* d_acc, double** d_res, size_t* res_bytes) {
    int rc;
    DiffractPlan pl;                                             // (members: strips of G waves; the LDS mode keeps the my totals of a strip there too)
    if ((rc = plan_diffract(h, who, r, t0, count, wx, wy, bx, by, m ? m->G : 1, m ? 1 : 0, &pl))) return rc;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (!d_acc && !d_dst && (rc = h->diff_out.reserve(h, pl.n_out))) return rc;
    double* d_out = d_acc ? d_acc : (d_dst ? d_dst : h->diff_out.p);
    MemberWeights mw;                                            // by value: the caller's array is not read after this function
    for (int g = 0; m && g < MEMBERS_MAX; ++g) mw.w[g] = g < m->G ? m->weights[g] : 0.0;
    with_int<DIFF_DIRECT, DIFF_SHFL, DIFF_LDS>(pl.mode, [&](auto mode) { with_bool(pl.vec, [&](auto vec) { with_bool(d_acc != nullptr, [&](auto acc) {
        constexpr int MODE = decltype(mode)::value;
        constexpr bool VEC = decltype(vec)::value, ACC = decltype(acc)::value;
        if (m) hipLaunchKernelGGL((diffract_members_kernel<MODE, VEC, ACC>), dim3(pl.grid), dim3(pl.threads), pl.lds, h->stream, (const float2*)r.p,
                                  (long long)r.R, (long long)t0, (int)count, (long long)r.ld, (int)wx, (int)wy, (int)bx, (int)by, (int)m->G, mw,
                                  (long long)pl.strips, (int)pl.per, d_out);
        else hipLaunchKernelGGL((diffract_kernel<MODE, VEC, ACC>), dim3(pl.grid), dim3(pl.threads), pl.lds, h->stream, (const float2*)r.p,
                                (long long)r.R, (long long)t0, (int)count, (long long)r.ld, (int)wx, (int)wy, (int)bx, (int)by, (long long)pl.strips,
                                (int)pl.per, d_out);
    }); }); });
    HIPCHK(h, hipGetLastError());
    if ((rc = mark_launch(h, K_OTHER))) return rc;
    h->ctr.algorithmic_bytes += 8ull * (uint64_t)r.K * (uint64_t)r.B * (uint64_t)count;
    *d_res = d_out; *res_bytes = pl.n_out * sizeof(double);
    return MSL_OK;
}

// G, the weights of a members call
static int check_members(msl_handle* h, const char* who, int32_t G, const double* weights) {
    if (!weights) return fail(h, MSL_ERR_INVALID, "%s: null argument", who);
    if (G < 1 || G > MSL_MEMBERS_MAX) return fail(h, MSL_ERR_INVALID, "%s: %d members outside [1, %d]", who, G, MSL_MEMBERS_MAX);
    for (int g = 0; g < G; ++g)
        if (!std::isfinite(weights[g]) || weights[g] < 0) return fail(h, MSL_ERR_INVALID, "%s: weight %d is negative or not finite", who, g);
    return MSL_OK;
}

// One call of the pattern pass for the four entry points msl_diffract, msl_dose_add (dose: into the dose accumulator) and their members
// variants (m): the argument and state checks, the members, the source rows (whole positions), the resident window, the accumulator's
// shape, then the timed launch.  `out`: the host array of the two calls that download, which the dose calls do not have.
static int pattern_call(msl_handle* h, const char* who, const void* d_src_c64, int64_t B, int64_t T, int64_t K, int64_t ld, int32_t t0, int32_t count,
                        int32_t wx, int32_t wy, int32_t bx, int32_t by, const Members* m, bool dose, double* out) {
    if (dose && !h) return fail(h, MSL_ERR_INVALID, "%s: null handle", who);
    if (!dose && (!h || !out)) return fail(h, MSL_ERR_INVALID, "%s: null argument", who);
    if (dose && h->dose_B == 0) return fail(h, MSL_ERR_STATE, "%s: no accumulator (call msl_dose_reset)", who);
    int rc;
    if (m && (rc = check_members(h, who, m->G, m->weights))) return rc;
    const bool resident = !d_src_c64;
    Rows r{d_src_c64, B, T, K, ld};
    if ((rc = resolve_rows(h, who, SRC_WAVEFUNCTION | SRC_FIRST_B, &r))) return rc;
    if (m && r.B % m->G) return fail(h, MSL_ERR_INVALID, "%s: %lld waves are no multiple of %d members", who, (long long)r.B, m->G);
    if (resident && (wx != h->wx / h->bx || wy != h->wy / h->by))
        return fail(h, MSL_ERR_INVALID, "%s: window %d x %d, the handle stores %d x %d", who, wx, wy, h->wx / h->bx, h->wy / h->by);
    if (dose) {
        if ((rc = check_window_bin(h, who, wx, wy, bx, by))) return rc;
        const int64_t n = m ? r.B / m->G : r.B;
        if (n > h->dose_B || wx / bx != h->dose_mx || wy / by != h->dose_my)
            return fail(h, MSL_ERR_INVALID, "%s: %lld %s of %d x %d detector pixels, the last msl_dose_reset sized %lld of %d x %d", who, (long long)n,
                        m ? "positions" : "probes", wx / bx, wy / by, (long long)h->dose_B, h->dose_mx, h->dose_my);
    }
    double* d_out = nullptr;
    size_t out_bytes = 0;
    if ((rc = begin_timed(h, 1)) || (rc = pattern_launch(h, who, r, t0, count, wx, wy, bx, by, m, nullptr, dose ? h->dose_acc.p : nullptr, &d_out, &out_bytes)))
        return rc;
    return dose ? MSL_OK : download_sync(h, out, d_out, out_bytes);
}

int msl_diffract(msl_handle* h, const void* d_src_c64, int64_t B, int64_t T, int64_t K, int64_t ld, int32_t t0, int32_t count, int32_t wx, int32_t wy,
                 int32_t bx, int32_t by, double* out) {
    return pattern_call(h, "msl_diffract", d_src_c64, B, T, K, ld, t0, count, wx, wy, bx, by, nullptr, false, out);
}

// ---- coherent frame sums (coherent.h) ---------------------------------------------------------------------
int msl_coherent_reset(msl_handle* h, int64_t B) {
    if (!h) return fail(h, MSL_ERR_INVALID, "msl_coherent_reset: null handle");
    if (B < 1) B = h->cfg.n_probes;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    h->coh_B = 0; h->coh_K = 0;
    const size_t n = (size_t)B * h->wpitch;
    int rc = h->coh_acc.reserve(h, n);
    if (rc) return rc;
    HIPCHK(h, hipMemsetAsync(h->coh_acc, 0, n * sizeof(double2), h->stream));
    h->coh_B = B;
    return MSL_OK;
}

int msl_coherent_add(msl_handle* h, const void* d_src_c64, int64_t B, int64_t T, int64_t K, int64_t ld, int32_t t0, int32_t count) {
    if (!h) return fail(h, MSL_ERR_INVALID, "msl_coherent_add: null handle");
    Rows r{d_src_c64, B, T, K, ld};
    int rc = resolve_rows(h, "msl_coherent_add", SRC_WAVEFUNCTION | SRC_FIRST_B, &r);
    if (rc) return rc;
    if (r.B > h->coh_B || r.K > (int64_t)h->wpitch)
        return fail(h, MSL_ERR_INVALID, "msl_coherent_add: %lld probes of %lld pixels, the last msl_coherent_reset sized %lld of up to %zu", (long long)r.B,
                    (long long)r.K, (long long)h->coh_B, h->wpitch);
    if (h->coh_K && r.K != h->coh_K)
        return fail(h, MSL_ERR_INVALID, "msl_coherent_add: rows of %lld pixels after rows of %lld (msl_coherent_reset starts a new sum)", (long long)r.K,
                    (long long)h->coh_K);
    if ((rc = check_slots(h, "msl_coherent_add", "frame slots", t0, count, r.R))) return rc;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    // 16-byte loads need every image to start on 16 bytes and to end with a whole column pair
    const bool vec = (r.ld % 2 == 0) && (r.K % 2 == 0) && (((uintptr_t)r.p & 15) == 0);
    const int64_t lanes = vec ? r.K / 2 : r.K;
    const dim3 grid((unsigned)((lanes + 255) / 256), (unsigned)std::min<int64_t>(r.B, 65535));
    if ((rc = begin_timed(h, 1))) return rc;
    with_bool(vec, [&](auto v) {
        hipLaunchKernelGGL(coherent_add_kernel<decltype(v)::value>, grid, dim3(256), 0, h->stream, (const float2*)r.p, (long long)r.B, (long long)r.R,
                           (long long)t0, (int)count, (long long)r.ld, (long long)r.K, (long long)h->wpitch, h->coh_acc.p);
    });
    HIPCHK(h, hipGetLastError());
    if ((rc = mark_launch(h, K_OTHER))) return rc;
    h->coh_K = r.K;
    h->ctr.algorithmic_bytes += (uint64_t)r.K * (uint64_t)r.B * (8ull * (uint64_t)count + 32ull);
    return MSL_OK;
}

int msl_coherent_finish(msl_handle* h, int64_t B, int32_t n, int32_t wx, int32_t wy, int32_t bx, int32_t by, double* out) {
    if (!h || !out) return fail(h, MSL_ERR_INVALID, "msl_coherent_finish: null argument");
    if (B < 1) B = h->coh_B;
    if (B < 1 || B > h->coh_B) return fail(h, MSL_ERR_INVALID, "msl_coherent_finish: %lld probes, the last msl_coherent_reset sized %lld", (long long)B, (long long)h->coh_B);
    if (n < 1) return fail(h, MSL_ERR_INVALID, "msl_coherent_finish: %d frames", n);
    int rc = check_window_bin(h, "msl_coherent_finish", wx, wy, bx, by);
    if (rc) return rc;
    const int64_t K = (int64_t)wx * wy;
    if (K > (int64_t)h->wpitch || (h->coh_K && K != h->coh_K))
        return fail(h, MSL_ERR_INVALID, "msl_coherent_finish: window %d x %d over rows of %lld pixels", wx, wy, (long long)(h->coh_K ? h->coh_K : (int64_t)h->wpitch));
    if ((int64_t)bx * by > 0x7fffffffLL) return fail(h, MSL_ERR_UNSUPPORTED, "msl_coherent_finish: more than 2^31 pixels per bin");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const int mx = wx / bx, my = wy / by;
    const int64_t bins = B * mx * my;
    if ((rc = h->diff_out.reserve(h, (size_t)bins))) return rc;  // the staging of msl_diffract: both calls leave it read
    int L = 1;                                                   // lanes per bin: the largest power of two <= min(64, bx * by)
    while (L < 64 && 2 * (int64_t)L <= (int64_t)bx * by) L *= 2;
    const int64_t blocks = (bins * L + 255) / 256;
    if (blocks > 0x7fffffffLL) return fail(h, MSL_ERR_UNSUPPORTED, "msl_coherent_finish: too many detector pixels");
    hipLaunchKernelGGL(coherent_finish_kernel, dim3((unsigned)blocks), dim3(256), 0, h->stream, h->coh_acc.p, (long long)h->wpitch, (long long)bins, (int)wy,
                       mx, my, (int)bx, (int)by, L, (double)n * (double)n, h->diff_out.p);
    HIPCHK(h, hipGetLastError());
    return download_sync(h, out, h->diff_out, (size_t)bins * sizeof(double));
}

// ---- finite dose (dose.h) ---------------------------------------------------------------------------------
int msl_dose_reset(msl_handle* h, int64_t B, int32_t mx, int32_t my) {
    if (!h) return fail(h, MSL_ERR_INVALID, "msl_dose_reset: null handle");
    if (B < 1) B = h->cfg.n_probes;
    if (mx < 1 || my < 1) return fail(h, MSL_ERR_INVALID, "msl_dose_reset: pattern of %d x %d pixels", mx, my);
    const int64_t K = (int64_t)mx * my;
    if (K > 0xffffffffLL || B > 0xffffffffLL) return fail(h, MSL_ERR_UNSUPPORTED, "msl_dose_reset: more than 2^32 pixels per pattern or probes");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    h->dose_B = 0; h->dose_K = 0;
    const size_t n = (size_t)B * (size_t)K;
    int rc = h->dose_acc.reserve(h, n);
    if (rc) return rc;
    HIPCHK(h, hipMemsetAsync(h->dose_acc, 0, n * sizeof(double), h->stream));
    h->dose_B = B; h->dose_K = K; h->dose_mx = mx; h->dose_my = my;
    return MSL_OK;
}

int msl_dose_add(msl_handle* h, const void* d_src_c64, int64_t B, int64_t T, int64_t K, int64_t ld, int32_t t0, int32_t count, int32_t wx, int32_t wy,
                 int32_t bx, int32_t by) {
    return pattern_call(h, "msl_dose_add", d_src_c64, B, T, K, ld, t0, count, wx, wy, bx, by, nullptr, true, nullptr);
}

// ---- member ensembles (ensemble.h) ------------------------------------------------------------------------
int msl_diffract_members(msl_handle* h, const void* d_src_c64, int64_t B, int64_t T, int64_t K, int64_t ld, int32_t t0, int32_t count, int32_t wx,
                         int32_t wy, int32_t bx, int32_t by, int32_t G, const double* weights, double* out) {
    const Members m{G, weights};
    return pattern_call(h, "msl_diffract_members", d_src_c64, B, T, K, ld, t0, count, wx, wy, bx, by, &m, false, out);
}

int msl_dose_add_members(msl_handle* h, const void* d_src_c64, int64_t B, int64_t T, int64_t K, int64_t ld, int32_t t0, int32_t count, int32_t wx,
                         int32_t wy, int32_t bx, int32_t by, int32_t G, const double* weights) {
    const Members m{G, weights};
    return pattern_call(h, "msl_dose_add_members", d_src_c64, B, T, K, ld, t0, count, wx, wy, bx, by, &m, true, nullptr);
}

// the draw of msl_dose_counts / msl_dose_frames into the count staging (the counts, then the flag word): checks, launch, no download
static int dose_draw(msl_handle* h, const char* who, int64_t* B, double scale, uint64_t seed, int64_t probe0) {
    if (h->dose_B == 0) return fail(h, MSL_ERR_STATE, "%s: no accumulator (call msl_dose_reset)", who);
    if (*B < 1) *B = h->dose_B;
    if (*B > h->dose_B) return fail(h, MSL_ERR_INVALID, "%s: %lld probes, the last msl_dose_reset sized %lld", who, (long long)*B, (long long)h->dose_B);
    if (!std::isfinite(scale) || scale < 0) return fail(h, MSL_ERR_INVALID, "%s: scale %g is not a finite number >= 0", who, scale);
    if (probe0 < 0 || probe0 + *B > 0x100000000LL)
        return fail(h, MSL_ERR_INVALID, "%s: probes [%lld, %lld) outside [0, 2^32)", who, (long long)probe0, (long long)(probe0 + *B));
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const int64_t n = *B * h->dose_K;
    const int64_t blocks = (n + 255) / 256;
    if (blocks > 0x7fffffffLL) return fail(h, MSL_ERR_UNSUPPORTED, "%s: too many detector pixels", who);
    int rc = h->dose_cnt.reserve(h, (size_t)n + 1);              // the counts, then the flag word
    if (rc) return rc;
    uint32_t* d_flag = h->dose_cnt.p + n;
    HIPCHK(h, hipMemsetAsync(d_flag, 0, sizeof(uint32_t), h->stream));
    if ((rc = begin_timed(h, 2))) return rc;
    hipLaunchKernelGGL(dose_counts_kernel, dim3((unsigned)blocks), dim3(256), 0, h->stream, (const double*)h->dose_acc.p, (long long)n, (long long)h->dose_K,
                       scale, (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)probe0, h->dose_cnt.p, d_flag);
    HIPCHK(h, hipGetLastError());
    return mark_launch(h, K_OTHER);
}

// what follows the draw: the downloads asked for (null: none), the flag word, one wait
static int dose_collect(msl_handle* h, const char* who, int64_t n, double scale, uint32_t* counts_out, double* intensity_out, uint16_t* frames_out) {
    uint32_t flag = 0;
    if (frames_out) HIPCHK(h, hipMemcpyAsync(frames_out, h->cam_frames.p, (size_t)n * sizeof(uint16_t), hipMemcpyDeviceToHost, h->stream));
    if (counts_out) HIPCHK(h, hipMemcpyAsync(counts_out, h->dose_cnt.p, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(&flag, h->dose_cnt.p + n, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    if (intensity_out) HIPCHK(h, hipMemcpyAsync(intensity_out, h->dose_acc.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (flag) return fail(h, MSL_ERR_INVALID, "%s: an expected count (accumulator x scale %g) is negative or not finite", who, scale);
    return MSL_OK;
}

int msl_dose_counts(msl_handle* h, int64_t B, double scale, uint64_t seed, int64_t probe0, uint32_t* counts_out, double* intensity_out) {
    if (!h || !counts_out) return fail(h, MSL_ERR_INVALID, "msl_dose_counts: null argument");
    int rc = dose_draw(h, "msl_dose_counts", &B, scale, seed, probe0);
    if (rc) return rc;
    return dose_collect(h, "msl_dose_counts", B * h->dose_K, scale, counts_out, intensity_out, nullptr);
}

// ---- detector response (camera.h) -------------------------------------------------------------------------
static int camera_class(int radius) { return radius <= 0 ? 0 : radius <= 1 ? 1 : radius <= 2 ? 2 : radius <= 4 ? 4 : CAM_RADIUS_MAX; }

int msl_set_camera(msl_handle* h, int32_t radius, const double* psf, double gain, double offset, double readout_noise, int32_t bits) {
    if (!h) return fail(h, MSL_ERR_INVALID, "msl_set_camera: null handle");
    if (radius < 0) { h->cam_radius = -1; return MSL_OK; }
    if (radius > CAM_RADIUS_MAX) return fail(h, MSL_ERR_INVALID, "msl_set_camera: radius %d is above %d", radius, CAM_RADIUS_MAX);
    if (!psf && radius != 0) return fail(h, MSL_ERR_INVALID, "msl_set_camera: no table for radius %d", radius);
    const int w = 2 * radius + 1;
    for (int i = 0; psf && i < w * w; ++i)
        if (!std::isfinite(psf[i]) || psf[i] < 0) return fail(h, MSL_ERR_INVALID, "msl_set_camera: weight %d (%g) is negative or not finite", i, psf[i]);
    if (!std::isfinite(gain) || !(gain > 0)) return fail(h, MSL_ERR_INVALID, "msl_set_camera: gain %g is not a finite number > 0", gain);
    if (!std::isfinite(offset) || offset < 0) return fail(h, MSL_ERR_INVALID, "msl_set_camera: offset %g is not a finite number >= 0", offset);
    if (!std::isfinite(readout_noise) || readout_noise < 0)
        return fail(h, MSL_ERR_INVALID, "msl_set_camera: readout noise %g is not a finite number >= 0", readout_noise);
    if (bits < 1 || bits > 16) return fail(h, MSL_ERR_INVALID, "msl_set_camera: %d bits, outside 1 .. 16", bits);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const int rc_ = camera_class(radius), wc = 2 * rc_ + 1;      // the table of the class: zero weights around the caller's
    std::vector<double> tab((size_t)wc * wc, 0.0);
    for (int a = 0; a < w; ++a)
        for (int b = 0; b < w; ++b) tab[(size_t)(a + rc_ - radius) * wc + (b + rc_ - radius)] = psf ? psf[a * w + b] + 0.0 : 1.0;
    h->cam_radius = -1;
    int rc = h->cam_psf.reserve(h, (size_t)(2 * CAM_RADIUS_MAX + 1) * (2 * CAM_RADIUS_MAX + 1));
    if (rc) return rc;
    HIPCHK(h, hipMemcpyAsync(h->cam_psf.p, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));                  // (tab leaves scope)
    h->cam_radius = radius; h->cam_class = rc_; h->cam_bits = bits;
    h->cam_gain = gain; h->cam_offset = offset; h->cam_noise = readout_noise;
    return MSL_OK;
}

// the camera pass over the B patterns of mx x my counts at the head of the count staging -> the frame staging; one launch
static int camera_launch(msl_handle* h, const char* who, int64_t B, int mx, int my, uint64_t seed, int64_t probe0) {
    CameraArgs g;
    g.tiles_x = (mx + CAM_TX - 1) / CAM_TX; g.tiles_y = (my + CAM_TY - 1) / CAM_TY;
    const int64_t per = (int64_t)g.tiles_x * g.tiles_y;
    if (per > 0x7fffffffLL || B > 0x7fffffffLL / per) return fail(h, MSL_ERR_UNSUPPORTED, "%s: too many detector pixels", who);
    int rc = h->cam_frames.reserve(h, (size_t)B * mx * my);
    if (rc) return rc;
    g.counts = h->dose_cnt.p; g.psf = h->cam_psf.p; g.frames = h->cam_frames.p;
    g.mx = mx; g.my = my;
    g.gain = h->cam_gain; g.offset = h->cam_offset; g.noise = h->cam_noise; g.full = (double)((1 << h->cam_bits) - 1);
    g.k0 = (uint32_t)seed; g.k1 = (uint32_t)(seed >> 32); g.probe0 = (uint32_t)probe0;
    const dim3 grid((unsigned)(B * per)), block(256);
    switch (h->cam_class) {
        case 0: hipLaunchKernelGGL(camera_frames_kernel<0>, grid, block, 0, h->stream, g); break;
        case 1: hipLaunchKernelGGL(camera_frames_kernel<1>, grid, block, 0, h->stream, g); break;
        case 2: hipLaunchKernelGGL(camera_frames_kernel<2>, grid, block, 0, h->stream, g); break;
        case 4: hipLaunchKernelGGL(camera_frames_kernel<4>, grid, block, 0, h->stream, g); break;
        default: hipLaunchKernelGGL(camera_frames_kernel<CAM_RADIUS_MAX>, grid, block, 0, h->stream, g); break;
    }
    HIPCHK(h, hipGetLastError());
    return mark_launch(h, K_OTHER);
}

int msl_camera_frames(msl_handle* h, const uint32_t* counts_host, int64_t B, int32_t mx, int32_t my, uint64_t seed, int64_t probe0, uint16_t* frames_out) {
    if (!h || !counts_host || !frames_out) return fail(h, MSL_ERR_INVALID, "msl_camera_frames: null argument");
    if (h->cam_radius < 0) return fail(h, MSL_ERR_STATE, "msl_camera_frames: no camera (call msl_set_camera)");
    if (B < 1 || mx < 1 || my < 1) return fail(h, MSL_ERR_INVALID, "msl_camera_frames: %lld patterns of %d x %d pixels", (long long)B, mx, my);
    if (probe0 < 0 || probe0 + B > 0x100000000LL)
        return fail(h, MSL_ERR_INVALID, "msl_camera_frames: probes [%lld, %lld) outside [0, 2^32)", (long long)probe0, (long long)(probe0 + B));
    const int64_t K = (int64_t)mx * my;
    if (K > 0xffffffffLL) return fail(h, MSL_ERR_UNSUPPORTED, "msl_camera_frames: more than 2^32 pixels per pattern");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const size_t n = (size_t)B * (size_t)K;
    int rc = h->dose_cnt.reserve(h, n + 1);                      // (sized as msl_dose_counts sizes it: the flag word behind the counts)
    if (rc) return rc;
    HIPCHK(h, hipMemcpyAsync(h->dose_cnt.p, counts_host, n * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    if ((rc = begin_timed(h, 1))) return rc;
    if ((rc = camera_launch(h, "msl_camera_frames", B, mx, my, seed, probe0))) return rc;
    return download_sync(h, frames_out, h->cam_frames.p, n * sizeof(uint16_t));
}

int msl_dose_frames(msl_handle* h, int64_t B, double scale, uint64_t seed, int64_t probe0, uint16_t* frames_out, uint32_t* counts_out_or_null,
                    double* intensity_out_or_null) {
    if (!h || !frames_out) return fail(h, MSL_ERR_INVALID, "msl_dose_frames: null argument");
    if (h->cam_radius < 0) return fail(h, MSL_ERR_STATE, "msl_dose_frames: no camera (call msl_set_camera)");
    int rc = dose_draw(h, "msl_dose_frames", &B, scale, seed, probe0);
    if (rc) return rc;
    if ((rc = camera_launch(h, "msl_dose_frames", B, h->dose_mx, h->dose_my, seed, probe0))) return rc;
    return dose_collect(h, "msl_dose_frames", B * h->dose_K, scale, counts_out_or_null, intensity_out_or_null, frames_out);
}

// ---- images through an objective lens (image.h) -----------------------------------------------------------
static int image_full_grid(msl_handle* h, const char* who) {
    if (h->wpix != (size_t)h->cfg.nx * h->cfg.ny || h->bx != 1 || h->by != 1)
        return fail(h, MSL_ERR_INVALID, "%s: the handle stores a k-window or bins; an image needs the full %d x %d spectrum", who, h->cfg.nx, h->cfg.ny);
    return MSL_OK;
}

int msl_image_reset(msl_handle* h, int64_t n_images) {
    if (!h) return fail(h, MSL_ERR_INVALID, "msl_image_reset: null handle");
    int rc = image_full_grid(h, "msl_image_reset");
    if (rc) return rc;
    if (n_images < 1) return fail(h, MSL_ERR_INVALID, "msl_image_reset: %lld images", (long long)n_images);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    h->img_n = 0;
    const size_t n = (size_t)n_images * h->cfg.nx * h->cfg.ny;
    if ((rc = h->img_acc.reserve(h, n))) return rc;
    HIPCHK(h, hipMemsetAsync(h->img_acc, 0, n * sizeof(double), h->stream));
    h->img_n = n_images;
    return MSL_OK;
}

int msl_image_add(msl_handle* h, const void* d_src_c64, int64_t B, int64_t T, int64_t ld, int32_t t0, int32_t count, const double* polar14x2,
                  double aperture_k, double weight, int64_t first, int64_t stride) {
    if (!h) return fail(h, MSL_ERR_INVALID, "msl_image_add: null handle");
    int rc = image_full_grid(h, "msl_image_add");
    if (rc) return rc;
    const msl_config& c = h->cfg;
    Rows r{d_src_c64, B, T, (int64_t)c.nx * c.ny, ld};
    if ((rc = resolve_rows(h, "msl_image_add", SRC_WAVEFUNCTION | SRC_FIRST_B, &r)) || (rc = check_slots(h, "msl_image_add", "frame slots", t0, count, r.R))) return rc;
    B = r.B; T = r.R; ld = r.ld;
    const int64_t K = r.K;
    if (!std::isfinite(weight) || !std::isfinite(aperture_k)) return fail(h, MSL_ERR_INVALID, "msl_image_add: weight or aperture is not finite");
    bool has_chi = false;
    for (int k = 0; polar14x2 && k < 28; ++k) {
        if (!std::isfinite(polar14x2[k])) return fail(h, MSL_ERR_INVALID, "msl_image_add: aberration value %d is not finite", k);
        if (!(k & 1) && polar14x2[k] != 0) has_chi = true;
    }
    if (first < 0 || stride < 0 || (stride == 0 && B > 1) || first + (B - 1) * stride >= h->img_n)
        return fail(h, MSL_ERR_INVALID, "msl_image_add: images %lld + b * %lld of %lld probes, the last msl_image_reset sized %lld", (long long)first,
                    (long long)stride, (long long)B, (long long)h->img_n);
    // the work buffer is psi: n_probes x frame batch images, which the slice loop has finished with
    const int64_t cap = (int64_t)c.n_probes * h->FB;
    if (B > cap) return fail(h, MSL_ERR_INVALID, "msl_image_add: %lld probes, the work buffer holds %lld images", (long long)B, (long long)cap);
    HIPCHK(h, hipSetDevice(c.device));
    const ProbeAberrations ab = has_chi ? probe_aberrations(polar14x2, c.wavelength) : ProbeAberrations{};
    const float2* src = (const float2*)r.p + (int64_t)t0 * ld;
    const bool pitch_even = h->pitch % 2 == 0;
    // 16-byte accesses: an even column maps to an even shifted column and the pair does not wrap (ny, ny / 2 even), every image and row starts on 16 bytes
    const bool vec_lens = c.ny % 4 == 0 && ld % 2 == 0 && pitch_even && (((uintptr_t)r.p & 15) == 0);
    const bool vec_acc = c.ny % 2 == 0 && pitch_even;
    const int64_t lanes_lens = (int64_t)c.nx * (vec_lens ? c.ny / 2 : c.ny), lanes_acc = (int64_t)c.nx * (vec_acc ? c.ny / 2 : c.ny);
    const unsigned gx_lens = (unsigned)((lanes_lens + 255) / 256), gx_acc = (unsigned)((lanes_acc + 255) / 256);
    const int64_t per = cap / B;                                 // frames per chunk
    const double radius = aperture_k > 0 ? aperture_k : 0.0;
    const float scale = 1.0f / ((float)c.nx * (float)c.ny);
    if ((rc = begin_timed(h, (int)std::min<int64_t>(8 * ((count + per - 1) / per), 4096)))) return rc;
    h->have_exit = false;                                        // MSL_BUF_EXIT is consumed
    h->pm_g = 0;
    for (int64_t j0 = 0; j0 < count; j0 += per) {
        const int64_t n = std::min<int64_t>(per, count - j0), images = n * B;
        // about 4096 workgroups: H is evaluated once per lane and reused for the images the lane walks
        const unsigned gy = (unsigned)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(images, 65535), (4096 + gx_lens - 1) / gx_lens));
        const float2* s = src + j0 * ld;
        with_bool(vec_lens, [&](auto v) {
            hipLaunchKernelGGL(lens_apply_kernel<decltype(v)::value>, dim3(gx_lens, gy), dim3(256), 0, h->stream, s, (long long)B, (long long)T, (long long)ld,
                               (long long)images, c.nx, c.ny, h->pitch, 1.0 / (c.nx * c.dx), 1.0 / (c.ny * c.dy), radius, c.wavelength, (int)has_chi, ab,
                               h->psi.p);
        });
        HIPCHK(h, hipGetLastError());
        if ((rc = mark_launch(h, K_OTHER))) return rc;
        if ((rc = fft2_inplace(h, h->psi, (int)images, -1, scale, h->pitch))) return rc;
        const dim3 grid_acc(gx_acc, (unsigned)std::min<int64_t>(B, 65535));
        with_bool(vec_acc, [&](auto v) {
            hipLaunchKernelGGL(image_accumulate_kernel<decltype(v)::value>, grid_acc, dim3(256), 0, h->stream, (const float2*)h->psi.p, (long long)B, (int)n,
                               c.nx, c.ny, h->pitch, weight, (long long)first, (long long)stride, h->img_acc.p);
        });
        HIPCHK(h, hipGetLastError());
        if ((rc = mark_launch(h, K_OTHER))) return rc;
    }
    h->ctr.algorithmic_bytes += (uint64_t)K * (uint64_t)B * (56ull * (uint64_t)count + 16ull);
    return MSL_OK;
}

int msl_image_download(msl_handle* h, int64_t first, int64_t n, double* out) {
    if (!h || !out) return fail(h, MSL_ERR_INVALID, "msl_image_download: null argument");
    if (first < 0 || n < 1 || first + n > h->img_n)
        return fail(h, MSL_ERR_INVALID, "msl_image_download: images [%lld,%lld), the last msl_image_reset sized %lld", (long long)first, (long long)(first + n),
                    (long long)h->img_n);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const size_t npix = (size_t)h->cfg.nx * h->cfg.ny;
    return download_sync(h, out, h->img_acc + (size_t)first * npix, (size_t)n * npix * sizeof(double));
}

int msl_tacaw_diffraction(msl_handle* h, const void* d_src_f32, int64_t B, int64_t F, int64_t K, int64_t ld, int64_t b0, int64_t b1,
                          int64_t f0, int64_t f1, double scale, double* out) {
    if (!out) return fail(h, MSL_ERR_INVALID, "msl_tacaw_diffraction: null output");
    Rows r{d_src_f32, B, F, K, ld};
    int rc = resolve_rows(h, "msl_tacaw_diffraction", SRC_INTENSITY | SRC_INT32_ROWS, &r);
    if (rc) return rc;
    B = r.B; F = r.R; K = r.K; ld = r.ld;
    if (b0 < 0 || b1 > B || b0 >= b1 || f0 < 0 || f1 > F || f0 >= f1)
        return fail(h, MSL_ERR_INVALID, "msl_tacaw_diffraction: range [%lld,%lld) x [%lld,%lld) outside (%lld,%lld)", (long long)b0,
                    (long long)b1, (long long)f0, (long long)f1, (long long)B, (long long)F);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if ((rc = h->scratch.reserve(h, (size_t)K * sizeof(double)))) return rc;
    double* d_out = (double*)h->scratch.p;
    const bool vec = (K % 4 == 0) && (ld % 4 == 0);
    const long long threads = vec ? K / 4 : K;
    const unsigned grid = (unsigned)((threads + 255) / 256);
    with_bool(vec, [&](auto v) {
        hipLaunchKernelGGL(reduce_bf_kernel<decltype(v)::value>, dim3(grid), dim3(256), 0, h->stream, (const float*)r.p, (long long)F, (long long)K,
                           (long long)ld, (long long)b0, (long long)b1, (long long)f0, (long long)f1, scale, d_out);
    });
    HIPCHK(h, hipGetLastError());
    return download_sync(h, out, d_out, (size_t)K * sizeof(double));
}

int msl_tacaw_dispersion(msl_handle* h, const void* d_src_f32, int64_t B, int64_t F, int64_t K, int64_t ld, const int64_t* idx, int64_t n, float* out) {
    if (!out || !idx) return fail(h, MSL_ERR_INVALID, "msl_tacaw_dispersion: null argument");
    Rows r{d_src_f32, B, F, K, ld};
    int rc = resolve_rows(h, "msl_tacaw_dispersion", SRC_INTENSITY | SRC_INT32_ROWS, &r);
    if (rc) return rc;
    B = r.B; F = r.R; K = r.K; ld = r.ld;
    if (n < 1) return fail(h, MSL_ERR_INVALID, "msl_tacaw_dispersion: empty path");
    for (int64_t i = 0; i < n; ++i)
        if (idx[i] < 0 || idx[i] >= K) return fail(h, MSL_ERR_INVALID, "msl_tacaw_dispersion: index %lld outside [0,%lld)", (long long)idx[i], (long long)K);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const size_t idx_bytes = (size_t)n * sizeof(int64_t), out_bytes = (size_t)B * F * n * sizeof(float);
    if ((rc = h->scratch.reserve(h, idx_bytes + out_bytes))) return rc;
    long long* d_idx = (long long*)h->scratch.p;
    float* d_out = (float*)(h->scratch + idx_bytes);
    HIPCHK(h, hipMemcpyAsync(d_idx, idx, idx_bytes, hipMemcpyHostToDevice, h->stream));
    const long long tot = (long long)B * F * n;
    hipLaunchKernelGGL(gather_k_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, h->stream, (const float*)r.p,
                       (long long)(B * F), (long long)ld, d_idx, (long long)n, d_out);
    HIPCHK(h, hipGetLastError());
    return download_sync(h, out, d_out, out_bytes);
}

int msl_download(msl_handle* h, msl_buffer what, void* dst, size_t bytes, int64_t first, int64_t count) {
    if (!h || !dst) return fail(h, MSL_ERR_INVALID, "msl_download: null argument");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const char* src = (const char*)msl_device_ptr(h, what);
    size_t total = msl_buffer_bytes(h, what);
    if (!src || total == 0) return fail(h, MSL_ERR_STATE, "msl_download: buffer %d not available", (int)what);
    if (what == MSL_BUF_EXIT && !h->have_exit) return fail(h, MSL_ERR_STATE, "msl_download: no exit waves (call msl_propagate)");
    if (what == MSL_BUF_TRANSMISSION && h->onepass && h->have_potential) {
        // the one-pass loop keeps every second slice transposed in its own buffer: restore the natural copies
        const int rc = restore_natural_slices(h, h->cur_batch);
        if (rc) return rc;
    }
    size_t off = 0, len = total;
    if (count > 0 && what != MSL_BUF_WAVEFUNCTION && what != MSL_BUF_INTENSITY)
        return fail(h, MSL_ERR_INVALID, "msl_download: ranges only for wavefunction/intensity");
    if (what == MSL_BUF_LAYERS) {
        // (L, P, T, wpitch) on the device -> dense (L, P, T, wx*wy) on the host
        const size_t rows = total / sizeof(float2) / h->wpitch;
        len = rows * h->wpix * sizeof(float2);
        if (bytes != len) return fail(h, MSL_ERR_INVALID, "msl_download: dst holds %zu bytes, buffer is %zu", bytes, len);
        HIPCHK(h, hipMemcpy2DAsync(dst, h->wpix * sizeof(float2), src, h->wpitch * sizeof(float2), h->wpix * sizeof(float2), rows,
                                   hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        return MSL_OK;
    }
    if (what == MSL_BUF_WAVEFUNCTION || what == MSL_BUF_INTENSITY) {
        // (P, rows, ld) on the device -> dense (P, rows, wx*wy) on the host
        const size_t es = what == MSL_BUF_WAVEFUNCTION ? sizeof(float2) : sizeof(float);
        const size_t ld = what == MSL_BUF_WAVEFUNCTION ? h->wpitch : h->intensity_ld;
        const size_t rows_per_probe = total / es / ld / h->cfg.n_probes;
        size_t n_probes = h->cfg.n_probes;
        if (count > 0) {
            if (first < 0 || first + count > h->cfg.n_probes) return fail(h, MSL_ERR_INVALID, "msl_download: probe range out of bounds");
            off = (size_t)first * rows_per_probe * ld * es; n_probes = (size_t)count;
        }
        const size_t rows = n_probes * rows_per_probe;
        len = rows * h->wpix * es;
        if (bytes != len) return fail(h, MSL_ERR_INVALID, "msl_download: dst holds %zu bytes, buffer slice is %zu", bytes, len);
        if (ld == h->wpix) {
            HIPCHK(h, hipMemcpyAsync(dst, src + off, len, hipMemcpyDeviceToHost, h->stream));
        } else {
            HIPCHK(h, hipMemcpy2DAsync(dst, h->wpix * es, src + off, ld * es, h->wpix * es, rows, hipMemcpyDeviceToHost, h->stream));
        }
        HIPCHK(h, hipStreamSynchronize(h->stream));
        return MSL_OK;
    }
    if (bytes != len) return fail(h, MSL_ERR_INVALID, "msl_download: dst holds %zu bytes, buffer slice is %zu", bytes, len);
    if ((what == MSL_BUF_PROBES || what == MSL_BUF_EXIT) && h->pitch != h->cfg.ny) {
        HIPCHK(h, hipMemcpy2DAsync(dst, (size_t)h->cfg.ny * sizeof(float2), src, (size_t)h->pitch * sizeof(float2),
                                   (size_t)h->cfg.ny * sizeof(float2), (size_t)h->cfg.n_probes * h->cfg.nx, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        return MSL_OK;
    }
    HIPCHK(h, hipMemcpyAsync(dst, src + off, len, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return MSL_OK;
}

static int frame_copy(msl_handle* h, int32_t slot, void* host, size_t bytes, bool to_host) {
    if (!h || !host) return fail(h, MSL_ERR_INVALID, "frame copy: null argument");
    if (!h->wf) return fail(h, MSL_ERR_STATE, "frame copy: handle created with n_frames == 0");
    const msl_config& c = h->cfg;
    if (slot < 0 || slot >= c.n_frames) return fail(h, MSL_ERR_INVALID, "frame copy: slot %d out of range [0,%d)", slot, c.n_frames);
    const size_t npix = h->wpix;                    // one (wx, wy) image of the stored window
    if (bytes != npix * c.n_probes * sizeof(float2)) return fail(h, MSL_ERR_INVALID, "frame copy: buffer holds %zu bytes, a frame is %zu", bytes, npix * c.n_probes * sizeof(float2));
    HIPCHK(h, hipSetDevice(c.device));
    // (P, T, wx, wy) device <-> (P, wx, wy) host: P strided blocks of one image
    float2* dev = h->wf + (size_t)slot * h->wpitch;
    if (to_host)
        HIPCHK(h, hipMemcpy2DAsync(host, npix * sizeof(float2), dev, (size_t)c.n_frames * h->wpitch * sizeof(float2), npix * sizeof(float2),
                                   c.n_probes, hipMemcpyDeviceToHost, h->stream));
    else
        HIPCHK(h, hipMemcpy2DAsync(dev, (size_t)c.n_frames * h->wpitch * sizeof(float2), host, npix * sizeof(float2), npix * sizeof(float2),
                                   c.n_probes, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return MSL_OK;
}

int msl_download_wavefunction_c128(msl_handle* h, int32_t n_frames_used, void* dst, size_t bytes) {
    if (!h || !dst) return fail(h, MSL_ERR_INVALID, "msl_download_wavefunction_c128: null argument");
    const msl_config& c = h->cfg;
    if (!h->wf) return fail(h, MSL_ERR_STATE, "msl_download_wavefunction_c128: no wavefunction buffer");
    if (n_frames_used < 1 || n_frames_used > c.n_frames) return fail(h, MSL_ERR_INVALID, "msl_download_wavefunction_c128: %d of %d frames", n_frames_used, c.n_frames);
    const size_t per_probe = (size_t)n_frames_used * h->wpix;
    if (bytes != (size_t)c.n_probes * per_probe * sizeof(double2))
        return fail(h, MSL_ERR_INVALID, "msl_download_wavefunction_c128: dst holds %zu bytes, the result has %zu", bytes, (size_t)c.n_probes * per_probe * sizeof(double2));
    HIPCHK(h, hipSetDevice(c.device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    // chunks of at most 256 MB of complex128 through the scratch buffer, probe by probe (a probe's used frames follow each other
    // at the image pitch); a chunk is a whole number of images or a piece of one
    size_t chunk = std::min<size_t>(per_probe, (size_t)(256u << 20) / sizeof(double2));
    if (chunk > h->wpix) chunk -= chunk % h->wpix;
    if (const char* e = dbg_env("MSL_C128_CHUNK")) chunk = std::max<size_t>(1, std::min<size_t>(chunk, (size_t)atoll(e)));      // (tests: several chunks per probe)
    int rc = h->scratch.reserve(h, chunk * sizeof(double2));
    if (rc) return rc;
    for (int p = 0; p < c.n_probes; ++p) {
        const float2* src = h->wf + (size_t)p * c.n_frames * h->wpitch;
        double2* out = (double2*)dst + (size_t)p * per_probe;
        for (size_t o = 0; o < per_probe; ) {
            // dense offset o = image o / wpix, pixel o % wpix; a piece that starts inside an image ends with it
            const size_t img = o / h->wpix, px = o % h->wpix;
            const size_t n = std::min(px ? std::min(chunk, h->wpix - px) : chunk, per_probe - o);
            const int grid = (int)std::min<size_t>((n + 255) / 256, (size_t)h->n_cus * 8);
            hipLaunchKernelGGL(widen_c64_kernel, dim3(grid), dim3(256), 0, h->stream, src + img * h->wpitch + px, (double2*)h->scratch.p, (long long)n,
                               (long long)h->wpix, (long long)h->wpitch);
            HIPCHK(h, hipGetLastError());
            HIPCHK(h, hipMemcpyAsync(out + o, h->scratch.p, n * sizeof(double2), hipMemcpyDeviceToHost, h->stream));
            HIPCHK(h, hipStreamSynchronize(h->stream));
            o += n;
        }
    }
    return MSL_OK;
}

int msl_set_layers(msl_handle* h, const int32_t* slices, int32_t n) {
    if (!h) return fail(h, MSL_ERR_INVALID, "null handle");
    const msl_config& c = h->cfg;
    if (n < 0 || (n > 0 && !slices)) return fail(h, MSL_ERR_INVALID, "msl_set_layers: %d slice indices", n);
    for (int i = 0; i < n; ++i) {
        if (slices[i] < 0 || slices[i] >= c.nz - 1)
            return fail(h, MSL_ERR_INVALID, "msl_set_layers: slice %d outside [0, %d) (the exit wave nz - 1 is always the last layer)", slices[i], c.nz - 1);
        if (i > 0 && slices[i] <= slices[i - 1]) return fail(h, MSL_ERR_INVALID, "msl_set_layers: slice indices must increase strictly");
    }
    if (!h->wf) return fail(h, MSL_ERR_STATE, "msl_set_layers: handle created with n_frames == 0");
    if (h->st_open) return fail(h, MSL_ERR_STATE, "msl_set_layers: a TACAW stream is open");
    if (h->lr_on) return fail(h, MSL_ERR_STATE, "msl_set_layers: the layers are reduced on the device (msl_set_layer_reduce): clear that mode first");
    HIPCHK(h, hipSetDevice(c.device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    const size_t block = layer_block_elems(h);
    const size_t images = (size_t)c.n_probes * h->FB;
    const size_t tap_elems = n > 0 ? (size_t)c.nx * h->pitch * images : 0;
    {
        size_t free_b = 0, total_b = 0;
        HIPCHK(h, hipMemGetInfo(&free_b, &total_b));
        const size_t have = free_b + (h->layers.n + h->tap.n) * 8;           // what the old result and tap give back
        const size_t need = block * 8 * (n + 1) + tap_elems * 8;
        if (need > have)
            return fail(h, MSL_ERR_NOMEM, "msl_set_layers: %d layers need %zu bytes, the device has %zu", n + 1, need, have);
    }
    // the old result goes first: at full size two of them would not fit
    h->layers.release();
    h->wf = nullptr;
    h->layer_slices.clear(); h->layer_block.clear();
    int rc = h->tap.alloc(h, tap_elems);
    if (!rc) rc = h->layers.alloc(h, block * (n + 1));
    if (rc) {                                                   // back to a single-layer result, if that still fits
        h->tap.release();
        if (h->layers.alloc(h, block) == MSL_OK) (void)hipMemsetAsync(h->layers, 0, block * sizeof(float2), h->stream);
        h->wf = h->layers;
        return fail(h, MSL_ERR_NOMEM, "msl_set_layers: %d layers of %zu bytes do not fit", n + 1, block * 8);
    }
    h->wf = h->layers + (size_t)n * block;
    if (n > 0) {
        h->layer_slices.assign(slices, slices + n);
        h->layer_block.assign(c.nz, -1);
        for (int i = 0; i < n; ++i) h->layer_block[slices[i]] = i;
    }
    HIPCHK(h, hipMemsetAsync(h->layers, 0, block * (n + 1) * sizeof(float2), h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return MSL_OK;
}

int msl_download_layers_c128(msl_handle* h, int32_t n_frames_used, void* dst, size_t bytes) {
    if (!h || !dst) return fail(h, MSL_ERR_INVALID, "msl_download_layers_c128: null argument");
    const msl_config& c = h->cfg;
    if (!h->wf) return fail(h, MSL_ERR_STATE, "msl_download_layers_c128: no wavefunction buffer");
    if (n_frames_used < 1 || n_frames_used > c.n_frames) return fail(h, MSL_ERR_INVALID, "msl_download_layers_c128: %d of %d frames", n_frames_used, c.n_frames);
    const int L = n_result_layers(h);
    const size_t per_probe = (size_t)n_frames_used * h->wpix;             // dense (T_used, wx*wy) offsets of a probe, L values each
    if (bytes != (size_t)c.n_probes * per_probe * L * sizeof(double2))
        return fail(h, MSL_ERR_INVALID, "msl_download_layers_c128: dst holds %zu bytes, the result has %zu", bytes, (size_t)c.n_probes * per_probe * L * sizeof(double2));
    HIPCHK(h, hipSetDevice(c.device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    const size_t block = layer_block_elems(h);
    // chunks of at most 256 MB of complex128 through the scratch buffer, as msl_download_wavefunction_c128
    size_t chunk = std::max<size_t>(1, std::min<size_t>(per_probe, (size_t)(256u << 20) / sizeof(double2) / L));
    if (const char* e = dbg_env("MSL_C128_CHUNK")) chunk = std::max<size_t>(1, std::min<size_t>(chunk, (size_t)atoll(e)));
    int rc = h->scratch.reserve(h, chunk * L * sizeof(double2));
    if (rc) return rc;
    for (int p = 0; p < c.n_probes; ++p) {
        double2* out = (double2*)dst + (size_t)p * per_probe * L;
        for (size_t o = 0; o < per_probe; o += chunk) {
            const size_t n = std::min(chunk, per_probe - o);
            const int grid = (int)std::min<size_t>((n * L + 255) / 256, (size_t)h->n_cus * 8);
            hipLaunchKernelGGL(layer_tap_c128_kernel, dim3(grid), dim3(256), 0, h->stream, h->layers.p, (double2*)h->scratch.p, (long long)o, (long long)n, L,
                               (long long)block, (long long)p * c.n_frames * h->wpitch, (long long)h->wpix, (long long)h->wpitch);
            HIPCHK(h, hipGetLastError());
            HIPCHK(h, hipMemcpyAsync(out + o * L, h->scratch, n * L * sizeof(double2), hipMemcpyDeviceToHost, h->stream));
            HIPCHK(h, hipStreamSynchronize(h->stream));
        }
    }
    return MSL_OK;
}

int msl_tacaw_layer(msl_handle* h, int32_t layer) {
    if (!h) return fail(h, MSL_ERR_INVALID, "null handle");
    if (!h->wf) return fail(h, MSL_ERR_STATE, "msl_tacaw_layer: no wavefunction buffer");
    const int L = n_result_layers(h);
    if (layer < 0 || layer >= L) return fail(h, MSL_ERR_INVALID, "msl_tacaw_layer: layer %d outside [0, %d)", layer, L);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    return tacaw_resident(h, h->layers + (size_t)layer * layer_block_elems(h));         // (the last block is wf)
}

int msl_tacaw_welch_layer(msl_handle* h, int32_t layer, int32_t L, int32_t hop, const double* window_L) {
    if (!h) return fail(h, MSL_ERR_INVALID, "null handle");
    if (!h->wf) return fail(h, MSL_ERR_STATE, "msl_tacaw_welch_layer: no wavefunction buffer");
    const int n = n_result_layers(h);
    if (layer < 0 || layer >= n) return fail(h, MSL_ERR_INVALID, "msl_tacaw_welch_layer: layer %d outside [0, %d)", layer, n);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    return welch_resident(h, h->layers + (size_t)layer * layer_block_elems(h), L, hop, window_L);         // (the last block is wf)
}

// ---- thickness series of the probe-batch modes: every tapped layer reduced at once (layer_reduce.h) ----------
namespace {

void lr_release(msl_handle* h) {
    h->lr_on = false; h->lr_what = 0; h->lr_count = 0;
    h->lr_block.release(); h->lr_stage.release(); h->tap.release();
    h->layer_slices.clear(); h->layer_block.clear();
}

// Everything of the sequence is sized at set-up (the staging, the partial slab of the detector tiles in h->scratch), so that no
// allocation -- which would wait for the device -- happens here.  The rows are all n_probes: a padded probe is reduced too.
int layer_reduce_queue(msl_handle* h, int l, const float2* block, int slot, int count) {
    const msl_config& c = h->cfg;
    const Rows r{block, c.n_probes, c.n_frames, (int64_t)h->wpix, (int64_t)h->wpitch};
    const LrLayout& y = h->lr_lay;
    int rc;
    // every write below is sized by the handle's detector and bin counts: they must still be the layout's (a failed msl_set_detectors
    // or msl_set_polar leaves none)
    if (((h->lr_what & LR_DETECT) && h->det_n != (int)y.D) || ((h->lr_what & LR_POLAR) && h->pol_bins != (int)y.n_bins))
        return fail(h, MSL_ERR_STATE, "msl_propagate_frames: %d detectors / %d polar bins, the layer reductions are set up for %d / %d", h->det_n,
                    h->pol_bins, (int)y.D, (int)y.n_bins);
    if (h->lr_what & LR_DETECT) {
        DetTiling t;
        if ((rc = plan_detect(h, "msl_propagate_frames", r, "frame slots", slot, count, &t, h->lr_stage + y.det(l))) ||
            (rc = detect_tiles(h, r, slot, count, t)) || (rc = mark_launch(h, K_OTHER)) || (rc = detect_finish(h, t)) || (rc = mark_launch(h, K_OTHER)))
            return rc;
        h->ctr.algorithmic_bytes += 8ull * (uint64_t)r.K * (uint64_t)r.B * (uint64_t)count;
    }
    double* d_res = nullptr;
    size_t bytes = 0;
    if (h->lr_what & LR_POLAR) {
        if ((rc = polar_launch(h, r, slot, count, h->lr_stage + y.pol(l), &d_res, &bytes)) || (rc = mark_launch(h, K_OTHER))) return rc;
        h->ctr.algorithmic_bytes += 8ull * (uint64_t)r.K * (uint64_t)r.B * (uint64_t)count;
    }
    if (h->lr_what & (LR_DIFFRACT | LR_PACBED)) {
        if ((rc = pattern_launch(h, "msl_diffract", r, slot, count, h->wx / h->bx, h->wy / h->by, h->lr_bx, h->lr_by, nullptr, h->lr_stage + y.diff(l), nullptr, &d_res, &bytes)))
            return rc;
    }
    h->lr_slot = slot; h->lr_count = count;
    return MSL_OK;
}

}  // namespace

int msl_set_layer_reduce(msl_handle* h, const int32_t* slices, int32_t n, uint32_t what, int32_t bx, int32_t by) {
    if (!h) return fail(h, MSL_ERR_INVALID, "null handle");
    const msl_config& c = h->cfg;
    if (n < 0 || (n > 0 && !slices)) return fail(h, MSL_ERR_INVALID, "msl_set_layer_reduce: %d slice indices", n);
    if (n_taps(h) > 0 && !h->lr_on) return fail(h, MSL_ERR_STATE, "msl_set_layer_reduce: the handle keeps layers (msl_set_layers): clear them first");
    HIPCHK(h, hipSetDevice(c.device));
    if (n == 0 || what == 0) {                                  // clearing: back to a plain handle
        HIPCHK(h, hipStreamSynchronize(h->stream));
        if (h->lr_on) lr_release(h);
        return MSL_OK;
    }
    if (what & ~(uint32_t)LR_ALL) return fail(h, MSL_ERR_INVALID, "msl_set_layer_reduce: unknown reduction bits 0x%x", what);
    for (int i = 0; i < n; ++i) {
        if (slices[i] < 0 || slices[i] >= c.nz - 1)
            return fail(h, MSL_ERR_INVALID, "msl_set_layer_reduce: slice %d outside [0, %d) (the exit wave nz - 1 is always the last layer)", slices[i], c.nz - 1);
        if (i > 0 && slices[i] <= slices[i - 1]) return fail(h, MSL_ERR_INVALID, "msl_set_layer_reduce: slice indices must increase strictly");
    }
    if (!h->wf) return fail(h, MSL_ERR_STATE, "msl_set_layer_reduce: handle created with n_frames == 0");
    if (h->st_open) return fail(h, MSL_ERR_STATE, "msl_set_layer_reduce: a TACAW stream is open");
    if ((what & LR_DETECT) && (h->det_n == 0 || h->det_K != h->wpix))
        return fail(h, MSL_ERR_STATE, "msl_set_layer_reduce: no detectors (call msl_set_detectors first)");
    if ((what & LR_POLAR) && (h->pol_bins == 0 || h->pol_K != h->wpix))
        return fail(h, MSL_ERR_STATE, "msl_set_layer_reduce: no bin map (call msl_set_polar first)");
    const bool patterns = what & (LR_DIFFRACT | LR_PACBED);
    const int sx = h->wx / h->bx, sy = h->wy / h->by;
    int rc;
    if (patterns && (rc = check_window_bin(h, "msl_set_layer_reduce", sx, sy, bx, by))) return rc;
    LrLayout y;
    if (!lr_layout(what, (int64_t)n + 1, c.n_probes, c.n_frames, h->det_n, h->pol_bins, patterns ? sx / bx : 0, patterns ? sy / by : 0, &y))
        return fail(h, MSL_ERR_INVALID, "msl_set_layer_reduce: %d layers of %d probes x %d frame slots are too large", n + 1, c.n_probes, c.n_frames);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    // new buffers first, the old state stays as it is until all of them exist
    DevBuf<float2> block, tap;
    DevBuf<double> stage;
    const size_t tap_elems = (size_t)c.nx * h->pitch * (size_t)c.n_probes * h->FB;
    const bool keep_tap = h->lr_on && h->tap.n == tap_elems;
    if ((rc = block.alloc(h, layer_block_elems(h))) || (!keep_tap && (rc = tap.alloc(h, tap_elems))) || (rc = stage.alloc(h, y.total)))
        return fail(h, MSL_ERR_NOMEM, "msl_set_layer_reduce: the layer block, the tap buffer and %zu bytes of staging do not fit", y.total * sizeof(double));
    if (what & LR_DETECT) {                                     // the partial slab of the detector tiles, for the largest sequence
        const DetTiling t = det_tiling((int64_t)c.n_probes * std::min(h->FB, c.n_frames), (int64_t)h->wpix, h->det_n);
        if ((rc = h->scratch.reserve(h, t.part_bytes))) return rc;
    }
    HIPCHK(h, hipMemsetAsync(block, 0, block.n * sizeof(float2), h->stream));
    HIPCHK(h, hipMemsetAsync(stage, 0, stage.n * sizeof(double), h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->lr_block = std::move(block);
    h->lr_stage = std::move(stage);
    if (!keep_tap) h->tap = std::move(tap);
    h->layer_slices.assign(slices, slices + n);
    h->layer_block.assign(c.nz, -1);
    for (int i = 0; i < n; ++i) h->layer_block[slices[i]] = i;
    h->lr_lay = y; h->lr_what = what; h->lr_bx = patterns ? bx : 1; h->lr_by = patterns ? by : 1;
    h->lr_count = 0;
    h->lr_on = true;
    return MSL_OK;
}

size_t msl_layer_reduce_bytes(const msl_handle* h, int32_t which) {
    if (!h || !h->lr_on) return 0;
    switch (which) {
        case MSL_LR_BYTES_BLOCK: return h->lr_block.n * sizeof(float2);
        case MSL_LR_BYTES_TAP: return h->tap.n * sizeof(float2);
        case MSL_LR_BYTES_STAGING: return h->lr_stage.n * sizeof(double);
    }
    return 0;
}

int msl_layer_fetch(msl_handle* h, int64_t B, int32_t count, double* det_out, double* polar_out, double* pattern_out) {
    if (!h) return fail(h, MSL_ERR_INVALID, "null handle");
    if (!h->lr_on) return fail(h, MSL_ERR_STATE, "msl_layer_fetch: no layer reductions (call msl_set_layer_reduce)");
    if (h->lr_count == 0) return fail(h, MSL_ERR_STATE, "msl_layer_fetch: no slice loop has run since msl_set_layer_reduce");
    if (count != h->lr_count) return fail(h, MSL_ERR_INVALID, "msl_layer_fetch: %d frames, the last sequence reduced %d", count, h->lr_count);
    if (B < 1) B = h->cfg.n_probes;
    if (B > h->cfg.n_probes) return fail(h, MSL_ERR_INVALID, "msl_layer_fetch: %lld probes, the handle has %d", (long long)B, h->cfg.n_probes);
    if ((det_out && !(h->lr_what & LR_DETECT)) || (polar_out && !(h->lr_what & LR_POLAR)) || (pattern_out && !(h->lr_what & LR_DIFFRACT)))
        return fail(h, MSL_ERR_INVALID, "msl_layer_fetch: an output whose reduction msl_set_layer_reduce did not ask for");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const LrLayout& y = h->lr_lay;
    const size_t rows = (size_t)B * count;
    for (int64_t l = 0; l < y.L; ++l) {
        if (det_out)
            HIPCHK(h, hipMemcpyAsync(det_out + (size_t)l * rows * y.D, h->lr_stage + y.det(l), rows * y.D * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        if (polar_out)
            HIPCHK(h, hipMemcpyAsync(polar_out + (size_t)l * rows * y.n_bins, h->lr_stage + y.pol(l), rows * y.n_bins * sizeof(double), hipMemcpyDeviceToHost,
                                     h->stream));
        if (pattern_out)
            HIPCHK(h, hipMemcpyAsync(pattern_out + (size_t)l * B * y.M, h->lr_stage + y.diff(l), (size_t)B * y.M * sizeof(double), hipMemcpyDeviceToHost,
                                     h->stream));
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return MSL_OK;
}

int msl_layer_pacbed_reset(msl_handle* h) {
    if (!h) return fail(h, MSL_ERR_INVALID, "null handle");
    if (!h->lr_on || !(h->lr_what & LR_PACBED)) return fail(h, MSL_ERR_STATE, "msl_layer_pacbed_reset: no accumulator (msl_set_layer_reduce with MSL_LR_PACBED)");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const LrLayout& y = h->lr_lay;
    HIPCHK(h, hipMemsetAsync(h->lr_stage + y.acc_off, 0, (size_t)y.L * y.M * sizeof(double), h->stream));
    return MSL_OK;
}

int msl_layer_pacbed_add(msl_handle* h, int64_t B) {
    if (!h) return fail(h, MSL_ERR_INVALID, "null handle");
    if (!h->lr_on || !(h->lr_what & LR_PACBED)) return fail(h, MSL_ERR_STATE, "msl_layer_pacbed_add: no accumulator (msl_set_layer_reduce with MSL_LR_PACBED)");
    if (h->lr_count == 0) return fail(h, MSL_ERR_STATE, "msl_layer_pacbed_add: no slice loop has run since msl_set_layer_reduce");
    if (B < 1) B = h->cfg.n_probes;
    if (B > h->cfg.n_probes) return fail(h, MSL_ERR_INVALID, "msl_layer_pacbed_add: %lld probes, the handle has %d", (long long)B, h->cfg.n_probes);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const LrLayout& y = h->lr_lay;
    if (y.L > 65535) return fail(h, MSL_ERR_UNSUPPORTED, "msl_layer_pacbed_add: more than 65535 layers");
    const double* src = h->lr_stage + y.diff_off;
    double* acc = h->lr_stage + y.acc_off;
    const bool pair = y.M % 2 == 0 && (((uintptr_t)src | (uintptr_t)acc) & 15) == 0;
    const long long lanes = pair ? y.M / 2 : y.M;
    int rc;
    if ((rc = begin_timed(h, 1))) return rc;
    with_bool(pair, [&](auto pr) {
        hipLaunchKernelGGL(pacbed_add_kernel<decltype(pr)::value>, dim3((unsigned)((lanes + 255) / 256), (unsigned)y.L), dim3(256), 0, h->stream, src, acc,
                           (int)B, (long long)y.P, (long long)y.M);
    });
    HIPCHK(h, hipGetLastError());
    if ((rc = mark_launch(h, K_OTHER))) return rc;
    h->ctr.algorithmic_bytes += 8ull * (uint64_t)y.L * (uint64_t)y.M * ((uint64_t)B + 2);
    return MSL_OK;
}

int msl_layer_pacbed_download(msl_handle* h, double* out) {
    if (!h || !out) return fail(h, MSL_ERR_INVALID, "msl_layer_pacbed_download: null argument");
    if (!h->lr_on || !(h->lr_what & LR_PACBED))
        return fail(h, MSL_ERR_STATE, "msl_layer_pacbed_download: no accumulator (msl_set_layer_reduce with MSL_LR_PACBED)");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const LrLayout& y = h->lr_lay;
    return download_sync(h, out, h->lr_stage + y.acc_off, (size_t)y.L * y.M * sizeof(double));
}

int msl_download_frame(msl_handle* h, int32_t slot, void* dst, size_t bytes) { return frame_copy(h, slot, dst, bytes, true); }
int msl_upload_frame(msl_handle* h, int32_t slot, const void* src, size_t bytes) { return frame_copy(h, slot, const_cast<void*>(src), bytes, false); }

int msl_synchronize(msl_handle* h) {
    if (!h) return fail(h, MSL_ERR_INVALID, "null handle");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return MSL_OK;
}

int msl_get_counters(const msl_handle* hc, msl_counters* out) {
    msl_handle* h = const_cast<msl_handle*>(hc);
    if (!h || !out) return fail(h, MSL_ERR_INVALID, "msl_get_counters: null argument");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    int rc = resolve_all(h);
    if (rc) return rc;
    h->ctr.slice_kernel_launches = h->n_kind[K_ROW] + h->n_kind[K_COL];
    h->ctr.ms_slice_kernels = h->ms_kind[K_ROW] + h->ms_kind[K_COL];
    h->ctr.row_launches = h->n_kind[K_ROW]; h->ctr.ms_row = h->ms_kind[K_ROW];
    h->ctr.col_launches = h->n_kind[K_COL]; h->ctr.ms_col = h->ms_kind[K_COL];
    *out = h->ctr;
    return MSL_OK;
}

int msl_reset_counters(msl_handle* h) {
    if (!h) return fail(h, MSL_ERR_INVALID, "null handle");
    int rc = resolve_all(h);
    if (rc) return rc;
    h->ctr = msl_counters{};
    for (int k = 0; k < K_NKINDS; ++k) { h->ms_kind[k] = 0; h->n_kind[k] = 0; }
    return MSL_OK;
}

int msl_fft2_host(msl_handle* h, const float* in, float* out, int32_t batch, int32_t dir) {
    if (!h || !in || !out) return fail(h, MSL_ERR_INVALID, "msl_fft2_host: null argument");
    if (batch < 1 || (dir != 1 && dir != -1)) return fail(h, MSL_ERR_INVALID, "msl_fft2_host: bad batch/dir");
    const msl_config& c = h->cfg;
    HIPCHK(h, hipSetDevice(c.device));
    const size_t n = (size_t)batch * c.nx * c.ny;
    DevBuf<float2> buf;
    int rc = buf.alloc(h, n);
    if (rc) return rc;
    HIPCHK(h, hipMemcpyAsync(buf, in, n * sizeof(float2), hipMemcpyHostToDevice, h->stream));
    h->cur = nullptr;
    rc = fft2_inplace(h, buf, batch, dir, dir < 0 ? 1.0f / ((float)c.nx * (float)c.ny) : 1.0f, c.ny);
    if (rc == MSL_OK) {
        hipError_t e = hipMemcpyAsync(out, buf, n * sizeof(float2), hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) rc = fail(h, MSL_ERR_HIP, "msl_fft2_host copy back: %s", hipGetErrorString(e));
    }
    return rc;
}

}  // extern "C"
