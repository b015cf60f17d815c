/* hermespy_rt.h -- the drop-in C ABI of the compute_paths hot path.
 *
 * libhermespy_rt_amd.so exports the three entry points the reference's callers bind
 * (its pybind11 module, compute_paths_pybind11.cpp:155-170, and its C demo, test/test.c:62-72):
 *
 *     compute_paths   replaces  inc/compute_paths.h:59-74  (impl src/compute_paths.c:419-757)
 *     scene_load      replaces  inc/scene.h:105            (impl src/scene.c:36-83)
 *     scene_save      replaces  inc/scene.h:95             (impl src/scene.c:7-34)
 *
 * with the same names, argument meaning, ownership and error behaviour, and the structs
 * below are byte-compatible with inc/vec3.h:6-8, inc/ray.h:6-9, inc/scene.h:10-32 and
 * inc/compute_paths.h:13-30.  A program compiled against the reference headers can be
 * re-linked against this library unchanged; a program may also include this header instead.
 *
 * What is different behind the boundary: the ray launch / triangle intersection / specular
 * bounce / scatter-to-RX loop runs as hand-written HIP kernels on an MI355X (gfx950).  There
 * is no CPU implementation in this library: without a usable HIP device compute_paths()
 * reports the HIP error on stderr and exits with status 70 (the reference's own "cannot
 * continue" status, src/compute_paths.c:504), and hrt_compute_paths_ex() returns the error.
 *
 * Plain C, no torch / HIP types in any signature.
 */
#ifndef HERMESPY_RT_H
#define HERMESPY_RT_H

#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- types (layout-identical to the reference headers) ---- */

typedef struct { float x, y, z; } Vec3;            /* inc/vec3.h:6-8   (12 bytes) */
typedef struct { Vec3 o, d; } Ray;                 /* inc/ray.h:6-9    (24 bytes) */

typedef struct {                                   /* inc/scene.h:10-27 */
    uint32_t num_vertices;
    Vec3 *vs;                 /* [num_vertices] */
    uint32_t num_triangles;
    uint32_t *is;             /* [num_triangles * 3] vertex indices */
    uint32_t material_index;  /* 0..16, ITU-R P.2040-3 table 3 row */
    Vec3 velocity;
    Vec3 *ns;                 /* [num_triangles] unit normals; NULL after scene_load.  As in
                                 the reference (src/compute_paths.c:212) compute_paths()
                                 malloc()s it and leaves it for free_scene(); like the
                                 reference it OVERWRITES the old pointer without freeing it
                                 (a hand-built Mesh may leave `ns` uninitialised): a caller
                                 that calls compute_paths() repeatedly on one Scene frees
                                 `ns` between the calls, or reloads the scene. */
} Mesh;

typedef struct { uint32_t num_meshes; Mesh *meshes; } Scene;   /* inc/scene.h:29-32 */

typedef struct {                                   /* inc/compute_paths.h:13-23 */
    uint32_t num_rays;
    Vec3 *directions_rx;      /* (num_rx, num_tx, num_rays) */
    Vec3 *directions_tx;      /* LoS: (num_rx, num_tx).  Scatter: NEVER written (as in the
                                 reference; callers allocate as little as num_rays Vec3) */
    float *a_te_re, *a_te_im, *a_tm_re, *a_tm_im;   /* (num_rx, num_tx, num_rays) */
    float *tau;               /* s */
    float *freq_shift;        /* Hz */
} ChannelInfo;

typedef struct {                                   /* inc/compute_paths.h:26-30 */
    uint32_t num_bounces, num_rays;
    Ray *rays;                /* scatter: >= num_tx*(num_bounces+1)*num_rays entries */
    uint8_t *rays_active;     /* scatter: >= (num_tx*num_bounces+1)*(num_rays/8+1) bytes */
} RaysInfo;

/* inc/scene.h:72-86 (static inline there too; everything the library stores in a Scene is
 * malloc()-compatible) */
static inline void free_mesh(Mesh *mesh) { free(mesh->vs); free(mesh->is); free(mesh->ns); }
static inline void free_scene(Scene *scene)
{
    for (uint32_t i = 0; i < scene->num_meshes; i++) free_mesh(&scene->meshes[i]);
    free(scene->meshes);
}

/* ---- the reference's entry points ---- */

/* Read a .hrt file.  Errors: perror + exit(8), as src/scene.c:36-83. */
Scene scene_load(const char *filepath);

/* Write a .hrt file (normals are not stored).  Errors: perror + exit(8). */
void scene_save(Scene *scene, const char *filepath);

/* Trace.  All out-arrays are caller-allocated; only the slots the reference writes are
 * written (dead rays' slots, blocked records' directions/freq_shift and the scatter
 * directions_tx stay untouched).  Scatter arrays are indexed
 * ((rx*num_tx + tx)*num_bounces + bounce)*num_rays + ray.  Blocking; not re-entrant. */
void compute_paths(Scene *scene, Vec3 *rx_pos, Vec3 *tx_pos, Vec3 *rx_vel, Vec3 *tx_vel,
                   float carrier_frequency_GHz, size_t num_rx, size_t num_tx, size_t num_rays,
                   size_t num_bounces, ChannelInfo *chanInfo_los, RaysInfo *raysInfo_los,
                   ChannelInfo *chanInfo_scat, RaysInfo *raysInfo_scat);

/* ---- additions (not in the reference) ---- */

/* Work counters of one call. */
typedef struct {
    uint64_t live[34];        /* live[b] = rays entering bounce b; live[num_bounces] = hits of
                                 the last bounce (valid for num_bounces <= 32) */
    uint64_t records;         /* scatter records written (hit x rx, blocked ones included) */
    uint64_t records_unblocked;
    uint64_t tests;           /* algorithmic ray-triangle tests of the brute-force reference:
                                 nrx*ntx*T + sum_b T*(live[b] + nrx*hits[b]) */
    double t_setup_s, t_launch_dirs_s, t_device_s, t_readback_s, t_total_s;   /* device / readback: the
                                 slowest device's */
    int device;               /* the first device used */
    int num_devices;          /* devices the batches were dealt to (HRT_DEVICES) */
    uint32_t num_batches;     /* round-robin shards of the launch set the call was cut into */
    /* per device d < num_devices (HRT_DEVICES order; at most 16): its id, the batches it took, the
     * time its thread spent waiting for its kernels and in readback + dense scatter -- on a node
     * with several GPUs these show the balance of the call */
    int dev_id[16];
    uint32_t dev_batches[16];
    double dev_t_device_s[16], dev_t_readback_s[16];
} hrt_stats;

/* Same as compute_paths() but returns 0 / a negative HRT_E_* code instead of exiting, takes
 * optional NULL for raysInfo_los / raysInfo_scat (skips their fill and transfer), and
 * reports counters.  `stats` may be NULL. */
int hrt_compute_paths_ex(Scene *scene, const Vec3 *rx_pos, const Vec3 *tx_pos,
                         const Vec3 *rx_vel, const Vec3 *tx_vel, float carrier_frequency_GHz,
                         size_t num_rx, size_t num_tx, size_t num_rays, size_t num_bounces,
                         ChannelInfo *chanInfo_los, RaysInfo *raysInfo_los,
                         ChannelInfo *chanInfo_scat, RaysInfo *raysInfo_scat, hrt_stats *stats);

/* hrt_compute_paths_ex for callers whose amplitudes are COMPLEX arrays (numpy complex64, C99 float
 * _Complex): a_te_re / a_te_im (a_tm_re / a_tm_im) of both ChannelInfo point at the real and the
 * imaginary part of element 0 of an interleaved array, element i being at [2 i] of each pointer.
 * The dense writer fills the complex arrays in place (the reference's planes would have to be
 * interleaved by the binding afterwards: compute_paths_pybind11.cpp:44-97 does).  Everything else
 * -- arguments, layout quirks, errors -- as hrt_compute_paths_ex. */
int hrt_compute_paths_interleaved(Scene *scene, const Vec3 *rx_pos, const Vec3 *tx_pos,
                                  const Vec3 *rx_vel, const Vec3 *tx_vel, float carrier_frequency_GHz,
                                  size_t num_rx, size_t num_tx, size_t num_rays, size_t num_bounces,
                                  ChannelInfo *chanInfo_los, RaysInfo *raysInfo_los,
                                  ChannelInfo *chanInfo_scat, RaysInfo *raysInfo_scat, hrt_stats *stats);

#define HRT_OK 0
#define HRT_E_INVALID (-1)   /* bad argument (zero count, material_index > 16, ...) */
#define HRT_E_NOMEM (-2)     /* host allocation failed */
#define HRT_E_HIP (-3)       /* HIP runtime error; text via hrt_last_error() */
#define HRT_E_CAPACITY (-4)  /* problem does not fit the device / > 71.5 M rays in one shard */

/* compute_paths() with the result as ONE list of path records instead of dense arrays: same inputs,
 * same tracing, the same values bit for bit (src/compute_paths.c:419-757), but only the records
 * that exist -- the dense [rx][tx][bounce][path] form is > 95 % unwritten slots.  Entry n is the
 * record the reference would write at scat.*[((rx[n]*num_tx + tx[n])*num_bounces + bounce[n])*
 * num_rays + path[n]]; order: by bounce, then rx, then the device's live-list order.
 * freq_shift = launch Doppler term of the ray minus the record's (the dense array's value for one
 * TX; the reference's dense fill is undefined for more).  All arrays are malloc'ed by the
 * call and released by hrt_path_list_free(). */
typedef struct {
    uint64_t num;
    uint32_t num_rx, num_tx;
    uint32_t *rx, *tx, *bounce;      /* [num] */
    uint64_t *path;                  /* [num] */
    float *a_te_re, *a_te_im, *a_tm_re, *a_tm_im, *tau;   /* [num]; a blocked record has zeros */
    Vec3 *direction_rx;              /* [num]; undefined for blocked records */
    float *freq_shift;               /* [num]; undefined for blocked records */
    uint8_t *unblocked;              /* [num] */
    uint32_t *mesh, *face;           /* [num] the triangle the ray left towards the RX */
    float *los;                      /* [num_rx*num_tx][8]: u32 status (0 coincident, 1 blocked,
                                      * 2 clear), a, tau, dir_tx xyz, freq_shift, - (HRT_LOS_*) */
} hrt_path_list;

/* include_blocked = 0 drops the blocked records (the reference writes zeros there). */
int hrt_compute_paths_list(Scene *scene, const Vec3 *rx_positions, const Vec3 *tx_positions,
                           const Vec3 *rx_velocities, const Vec3 *tx_velocities,
                           float carrier_frequency_GHz, size_t num_rx, size_t num_tx, size_t num_rays,
                           size_t num_bounces, int include_blocked, hrt_path_list *out,
                           hrt_stats *stats);
void hrt_path_list_free(hrt_path_list *list);

/* Channel frequency responses of the traced paths, formed on the device (include/hrt_device.h: hrt_channel).
 * For every (rx, tx), polarisation pol (0 = TE, 1 = TM), time sample m < num_times and frequency k < num_freqs:
 *     H[rx][tx][pol][m][k] = sum_p a_p^pol exp(j 2 pi (nu_p t_m - f_k tau_p)),  f_k = f0 + k df (Hz),  t_m = t0 + m dt (s)
 * over the paths of that link the caller selects in `parts`:
 *   HRT_CHANNEL_LOS      the LoS entry as the dense LoS output defines it: coincident a = 1, tau = nu = 0; blocked
 *                        a = 0; clear a = HRT_LOS_A (TE = TM, real), tau = HRT_LOS_TAU, nu = HRT_LOS_FS;
 *   HRT_CHANNEL_SCATTER  every scatter record of every bounce: a = the record's a_te / a_tm, tau = its tau,
 *                        nu = freq_shift as hrt_compute_paths_list reports it; blocked records add nothing.
 * The inputs of the sum are bit for bit the floats compute_paths returns.  The amplitudes carry no carrier phase
 * (the reference accumulates gains and delays separately), so f_k is an ABSOLUTE frequency: the baseband response
 * of an OFDM grid is f0 = carrier + offset of the first subcarrier.
 * out: complex [num_rx][num_tx][2][num_times][num_freqs], re/im interleaved (numpy complex64).
 * hrt_compute_channel traces like hrt_compute_paths_list (same batches, same device launch tables) and copies
 * only `out` back.  HRT_E_INVALID: num_freqs or num_times 0, num_freqs * num_times > 2^20, parts 0 or with unknown
 * bits, f0 / df / t0 / dt not finite. */
#define HRT_CHANNEL_LOS 1u
#define HRT_CHANNEL_SCATTER 2u
typedef struct {
    double f0_hz, df_hz;  uint32_t num_freqs;   /* f_k = f0 + k*df */
    double t0_s, dt_s;    uint32_t num_times;   /* t_m = t0 + m*dt */
    uint32_t parts;                             /* HRT_CHANNEL_LOS | HRT_CHANNEL_SCATTER */
} hrt_channel_spec;
int hrt_compute_channel(Scene *scene, const Vec3 *rx_pos, const Vec3 *tx_pos, const Vec3 *rx_vel,
                        const Vec3 *tx_vel, float carrier_frequency_GHz, size_t num_rx, size_t num_tx,
                        size_t num_rays, size_t num_bounces, const hrt_channel_spec *spec,
                        float *out /* complex interleaved, layout above */, hrt_stats *stats);

/* Antenna-array (MIMO) channel responses of the traced paths, formed on the device (include/hrt_device.h:
 * hrt_array_channel).  One array geometry is shared by all RX and one by all TX: element i < Nr of an RX sits at
 * offset r_i (metres, scene coordinates) from the traced RX position, element j < Nt of a TX at q_j from the
 * traced TX position.  Elements are isotropic.  For every link, polarisation (0 = TE, 1 = TM) and grid point:
 *     H[rx][tx][i][j][pol][m][k] = sum_p a_p^pol exp(j 2 pi (nu_p t_m - f_k tau_p))
 *                                        * exp(j 2 pi f_a (r_i . u_p^rx + q_j . u_p^tx) / c)
 * over the paths hrt_channel sums (the same parts, LoS and scatter terms; blocked records add nothing), c =
 * 299 792 458 m/s.  u^rx is the arrival direction as the dense output defines directions_rx: a unit vector from
 * the RX back along the incoming path.  u^tx is the departure direction: for the LoS entry directions_tx (the
 * coincident case too: u^rx = (1, 0, 0), u^tx = (-1, 0, 0)); for a scatter record the launch direction of its ray
 * (RaysInfo bounce 0).  The reference never writes directions_tx of scatter paths; this is the direction it
 * would hold.  The steering phase is narrowband: it is evaluated at the array frequency f_a, not at each f_k, so
 * it is off by at most 2 pi |f_k - f_a| max(|r_i| + |q_j|) / c.  With Nr = Nt = 1 and zero offsets the result is
 * hrt_compute_channel's, and the layout reduces to its layout.
 * out: complex [num_rx][num_tx][Nr][Nt][2][num_times][num_freqs], re/im interleaved (numpy complex64).
 * rx_elements / tx_elements: HOST arrays of Nr / Nt offsets.  Traced and batched like hrt_compute_channel; only
 * `out` is copied back.  HRT_E_INVALID, before the device is touched: every hrt_channel_spec check; Nr or Nt
 * outside 1..1024; Nr * Nt * num_times * num_freqs > 2^24; an offset or f_a not finite; f_a <= 0. */
int hrt_compute_array_channel(Scene *scene, const Vec3 *rx_pos, const Vec3 *tx_pos, const Vec3 *rx_vel,
                              const Vec3 *tx_vel, float carrier_frequency_GHz, size_t num_rx, size_t num_tx,
                              size_t num_rays, size_t num_bounces, const hrt_channel_spec *spec,
                              const Vec3 *rx_elements, size_t num_rx_elements, const Vec3 *tx_elements,
                              size_t num_tx_elements, double array_frequency_hz,
                              float *out /* complex interleaved, layout above */, hrt_stats *stats);

/* Beamformed (codebook) channel responses of the traced paths, formed on the device (include/hrt_device.h:
 * hrt_beam_channel): the channel after a combiner and a precoder from a codebook.  For every link, RX beam a < Br,
 * TX beam b < Bt, polarisation and grid point:
 *     B[rx][tx][a][b][pol][m][k] = sum_p a_p^pol exp(j 2 pi (nu_p t_m - f_k tau_p)) g_rx[a](u_p^rx) g_tx[b](u_p^tx)
 *     g_rx[a](u) = sum_i conj(W_rx[a][i]) exp(j 2 pi f_a r_i . u / c)      (combiner  w^H)
 *     g_tx[b](u) = sum_j      W_tx[b][j]  exp(j 2 pi f_a q_j . u / c)      (precoder  f)
 * which is sum_ij conj(W_rx[a][i]) H[rx][tx][i][j][pol][m][k] W_tx[b][j] with hrt_compute_array_channel's H for the
 * same elements and f_a: the paths, parts, u^rx and u^tx are exactly its.  The weights are folded into each path's
 * steering term, so H is never formed: the cost follows Br * Bt, not Nr * Nt, and Nr * Nt is not limited.  One
 * codebook is shared by all RX and one by all TX (as the element geometries are); the weights are not normalised.
 * out: complex [num_rx][num_tx][Br][Bt][2][num_times][num_freqs], re/im interleaved (numpy complex64).
 * rx_elements / tx_elements: HOST arrays of Nr / Nt offsets; rx_weights / tx_weights: HOST arrays [Br][Nr][2] /
 * [Bt][Nt][2] of (re, im) floats (numpy complex64 (Br, Nr) / (Bt, Nt)).  Traced and batched like hrt_compute_channel;
 * only `out` is copied back.  HRT_E_INVALID, before the device is touched: every hrt_channel_spec check; Nr or Nt
 * outside 1..256; Br or Bt outside 1..256; Br * Bt * num_times * num_freqs > 2^24; an offset, a weight or f_a not
 * finite; f_a <= 0; a NULL pointer. */
int hrt_compute_beam_channel(Scene *scene, const Vec3 *rx_pos, const Vec3 *tx_pos, const Vec3 *rx_vel,
                             const Vec3 *tx_vel, float carrier_frequency_GHz, size_t num_rx, size_t num_tx,
                             size_t num_rays, size_t num_bounces, const hrt_channel_spec *spec,
                             const Vec3 *rx_elements, size_t num_rx_elements, const Vec3 *tx_elements,
                             size_t num_tx_elements, double array_frequency_hz, const float *rx_weights,
                             size_t num_rx_beams, const float *tx_weights, size_t num_tx_beams,
                             float *out /* complex interleaved, layout above */, hrt_stats *stats);

/* Sampled channel impulse responses (taps) of the traced paths, formed on the device (include/hrt_device.h:
 * hrt_taps).  For every (rx, tx), polarisation pol (0 = TE, 1 = TM), time sample m < num_times and tap i < num_taps:
 *     h[rx][tx][pol][m][i] = sum_p a_p^pol exp(j 2 pi (nu_p t_m - f_c tau_p)) sinc(l_i - f_s tau_p)
 *     t_m = t0 + m dt (s),  l_i = l_min + i,  sinc(x) = sin(pi x) / (pi x),  sinc(0) = 1
 * over the paths hrt_channel sums (the same parts, LoS and scatter terms; blocked records add nothing).  f_s is the
 * sampling rate; f_c the frequency the baseband is taken around (the amplitudes carry no carrier phase, so f_c = 0
 * gives the raw sum).  This is the band-limited discrete-time channel: for |f| < f_s / 2 its DTFT
 * sum_i h[i] exp(-j 2 pi f l_i / f_s) is hrt_compute_channel's H at f_k = f_c + f.
 * out: complex [num_rx][num_tx][2][num_times][num_taps], re/im interleaved (numpy complex64).
 * hrt_compute_taps traces and batches like hrt_compute_channel (one device, one download at the end).
 * HRT_E_INVALID, before the device is touched: num_taps or num_times 0; num_taps * num_times > 2^20; f_s not finite
 * or <= 0; f_c, t0 or dt not finite; |l_min| or |l_min + num_taps| > 2^24; parts 0 or with unknown bits. */
typedef struct {
    double fs_hz, fc_hz;                        /* sampling rate, baseband centre frequency */
    double t0_s, dt_s;                          /* t_m = t0 + m*dt */
    int32_t l_min;  uint32_t num_taps;          /* l_i = l_min + i */
    uint32_t num_times;
    uint32_t parts;                             /* HRT_CHANNEL_LOS | HRT_CHANNEL_SCATTER */
} hrt_taps_spec;
int hrt_compute_taps(Scene *scene, const Vec3 *rx_pos, const Vec3 *tx_pos, const Vec3 *rx_vel,
                     const Vec3 *tx_vel, float carrier_frequency_GHz, size_t num_rx, size_t num_tx,
                     size_t num_rays, size_t num_bounces, const hrt_taps_spec *spec,
                     float *out /* complex interleaved, layout above */, hrt_stats *stats);

/* Antenna-array (MIMO) sampled impulse responses of the traced paths, formed on the device (include/hrt_device.h:
 * hrt_array_taps): the taps of hrt_compute_taps between the elements of hrt_compute_array_channel's arrays.  For every
 * link, element pair (i, j), polarisation pol (0 = TE, 1 = TM), time sample m < num_times and tap l < num_taps:
 *     h[rx][tx][i][j][pol][m][l] = sum_p a_p^pol exp(j 2 pi (nu_p t_m - f_c tau_p))
 *                                         * exp(j 2 pi f_a (r_i . u_p^rx + q_j . u_p^tx) / c) sinc(l_min + l - f_s tau_p)
 *     t_m = t0 + m dt,  sinc(x) = sin(pi x) / (pi x),  sinc(0) = 1,  c = 299 792 458 m/s
 * over the paths hrt_channel sums (the same parts, LoS and scatter terms; blocked records add nothing).  u^rx is
 * directions_rx; u^tx the launch direction of the record's ray; the LoS entry has u^tx = HRT_LOS_DIR and u^rx = -u^tx
 * (coincident: u^rx = (1, 0, 0), u^tx = (-1, 0, 0)), a real amplitude and TE = TM.  The steering is narrowband, as in
 * hrt_compute_array_channel: evaluated at f_a; one geometry is shared by all RX and one by all TX; the elements are
 * isotropic.  Identities: for |f| < f_s / 2 the DTFT sum_l h[..., l] exp(-j 2 pi f (l_min + l) / f_s) is
 * hrt_compute_array_channel's H at f_k = f_c + f (same f_a and elements), up to the taps cut off by the window; with
 * Nr = Nt = 1 and zero offsets the result is hrt_compute_taps's; pair (i, j) is a call with the single pair (r_i, q_j).
 * out: complex [num_rx][num_tx][Nr][Nt][2][num_times][num_taps], re/im interleaved (numpy complex64).
 * rx_elements / tx_elements: HOST arrays of Nr / Nt offsets.  Traced and batched like hrt_compute_channel; only `out`
 * is copied back.  HRT_E_INVALID, before the device is touched: every hrt_taps_spec check; Nr or Nt outside 1..1024;
 * Nr * Nt * num_times * num_taps > 2^24; an offset or f_a not finite; f_a <= 0. */
int hrt_compute_array_taps(Scene *scene, const Vec3 *rx_pos, const Vec3 *tx_pos, const Vec3 *rx_vel,
                           const Vec3 *tx_vel, float carrier_frequency_GHz, size_t num_rx, size_t num_tx,
                           size_t num_rays, size_t num_bounces, const hrt_taps_spec *spec,
                           const Vec3 *rx_elements, size_t num_rx_elements, const Vec3 *tx_elements,
                           size_t num_tx_elements, double array_frequency_hz,
                           float *out /* complex interleaved, layout above */, hrt_stats *stats);

/* Beamformed (codebook) sampled impulse responses of the traced paths, formed on the device (include/hrt_device.h:
 * hrt_beam_taps): the taps after a combiner and a precoder from a codebook.  For every link, RX beam a < Br, TX beam
 * b < Bt, polarisation, time sample m < num_times and tap l < num_taps:
 *     h[rx][tx][a][b][pol][m][l] = sum_p a_p^pol exp(j 2 pi (nu_p t_m - f_c tau_p)) g_rx[a](u_p^rx) g_tx[b](u_p^tx)
 *                                         * sinc(l_min + l - f_s tau_p)
 *     g_rx[a](u) = sum_i conj(W_rx[a][i]) exp(j 2 pi f_a r_i . u / c)      (combiner  w^H)
 *     g_tx[b](u) = sum_j      W_tx[b][j]  exp(j 2 pi f_a q_j . u / c)      (precoder  f)
 * which is sum_ij conj(W_rx[a][i]) h[rx][tx][i][j][pol][m][l] W_tx[b][j] with hrt_compute_array_taps's h for the same
 * elements and f_a: the paths, parts, u^rx, u^tx and the sinc rules are exactly its, the gains hrt_compute_beam_channel's.
 * The weights are folded into each path's steering term, so h is never formed: the cost follows Br * Bt, not Nr * Nt,
 * and Nr * Nt is not limited.  (An inverse FFT of hrt_compute_beam_channel aliases every delay beyond 1 / df; the
 * weights cannot be applied to finished taps of single antennas, because the gain differs per path.)
 * out: complex [num_rx][num_tx][Br][Bt][2][num_times][num_taps], re/im interleaved (numpy complex64).
 * rx_elements / tx_elements: HOST arrays of Nr / Nt offsets; rx_weights / tx_weights: HOST arrays [Br][Nr][2] /
 * [Bt][Nt][2] of (re, im) floats.  Traced and batched like hrt_compute_channel; only `out` is copied back.
 * HRT_E_INVALID, before the device is touched: every hrt_taps_spec check; Nr or Nt outside 1..256; Br or Bt outside
 * 1..256; Br * Bt * num_times * num_taps > 2^24; an offset, a weight or f_a not finite; f_a <= 0; a NULL pointer. */
int hrt_compute_beam_taps(Scene *scene, const Vec3 *rx_pos, const Vec3 *tx_pos, const Vec3 *rx_vel,
                          const Vec3 *tx_vel, float carrier_frequency_GHz, size_t num_rx, size_t num_tx,
                          size_t num_rays, size_t num_bounces, const hrt_taps_spec *spec,
                          const Vec3 *rx_elements, size_t num_rx_elements, const Vec3 *tx_elements,
                          size_t num_tx_elements, double array_frequency_hz, const float *rx_weights,
                          size_t num_rx_beams, const float *tx_weights, size_t num_tx_beams,
                          float *out /* complex interleaved, layout above */, hrt_stats *stats);

/* Received signals: the traced taps applied to baseband waveforms on the device (include/hrt_device.h: hrt_propagate),
 * what a link-level simulator's Channel.propagate(signal) returns.  With h the output of hrt_compute_array_taps
 * (hrt_compute_taps: Nr = Nt = 1; hrt_compute_beam_taps: beams in place of elements) and x the samples of every TX
 * port at the rate f_s, for every rx, RX element i, polarisation pol and output sample n < num_out:
 *     y[rx][i][pol][n] = sum_tx sum_j sum_{l < num_taps} h[rx][tx][i][j][pol][m(n)][l] x[tx][j][n - l_min - l]
 *     m(n) = min(n / samples_per_block, num_times - 1)     (integer division)
 * with x[..][k] = 0 for k < 0 or k >= num_samples; the index n - l_min - l is formed in 64-bit signed arithmetic.  The
 * sum over TX is part of the definition: a receiver hears all transmitters.  The channel varies block-wise in the
 * observation time: the taps of block m are meant to be formed at the centre of the block, t0 = t_start + (S - 1) /
 * (2 f_s), dt = S / f_s.  S = 1 with num_times = num_out is the per-sample time-variant channel, num_times = 1 the
 * time-invariant one; blocks past the last sample are not read.
 * x: complex [num_tx][Nt][num_samples]; y: complex [num_rx][Nr][2][num_out]; both re/im interleaved (numpy complex64).
 * The products and sums are float (f32 MFMA where num_times = 1 or samples_per_block is a multiple of 16, an fmaf
 * chain otherwise), every output summed in one fixed order: two calls give the same bits.  Non-finite taps or samples
 * give an undefined result.
 * hrt_compute_received_signal traces and batches exactly as hrt_compute_array_taps does, keeps the accumulated taps on
 * the device, uploads x (HOST) and runs the propagation once after the last batch; only y is copied back.
 * HRT_E_INVALID, before the device is touched: every refusal of hrt_compute_array_taps; a NULL x or y; every refusal
 * of hrt_propagate (include/hrt_device.h); spec->num_times != ceil(num_out / samples_per_block). */
typedef struct {
    uint32_t num_rx, num_tx;                    /* receivers, transmitters */
    uint32_t nr, nt;                            /* RX / TX elements (or beams) per link */
    uint32_t num_times, num_taps;               /* M blocks, L taps */
    int32_t l_min;                              /* tap l has the delay (l_min + l) / f_s */
    uint32_t samples_per_block;                 /* S */
    uint64_t num_samples, num_out;              /* N samples of x per port, N_out samples of y per row */
} hrt_propagate_spec;
uint64_t hrt_propagate_out_floats(const hrt_propagate_spec *spec);   /* num_rx nr 2 num_out 2; 0 for NULL */
int hrt_compute_received_signal(Scene *scene, const Vec3 *rx_pos, const Vec3 *tx_pos, const Vec3 *rx_vel,
                                const Vec3 *tx_vel, float carrier_frequency_GHz, size_t num_rx, size_t num_tx,
                                size_t num_rays, size_t num_bounces, const hrt_taps_spec *spec,
                                const Vec3 *rx_elements, size_t num_rx_elements, const Vec3 *tx_elements,
                                size_t num_tx_elements, double array_frequency_hz, uint32_t samples_per_block,
                                const float *x /* host, complex [num_tx][Nt][num_samples] */, uint64_t num_samples,
                                uint64_t num_out, float *y /* host, complex [num_rx][Nr][2][num_out] */,
                                hrt_stats *stats);

/* Per-point MIMO SVD of the array channel, formed on the device (include/hrt_device.h: hrt_channel_svd).  For every
 * link, polarisation, time sample and frequency, one "point" is the SVD of the Nr x Nt matrix
 * H[rx][tx][:][:][pol][m][k] of hrt_compute_array_channel's layout.  With n = min(Nr, Nt) the outputs keep that axis
 * order (the point axes innermost), in one flat buffer of hrt_svd_out_bytes bytes, the regions in this order (a region
 * not asked for in `want` is absent, size 0):
 *   sigma   float  [num_rx][num_tx][n][2][T][K]        descending in the n axis, >= 0
 *   u       complex [num_rx][num_tx][Nr][n][2][T][K]   left vectors   (HRT_SVD_U)
 *   v       complex [num_rx][num_tx][Nt][n][2][T][K]   right vectors  (HRT_SVD_V)
 *   sweeps  uint32 [num_rx][num_tx][2][T][K]           Jacobi sweeps that rotated; HRT_SVD_NOT_CONVERGED at the cap
 *   H = u diag(sigma) v^H
 * Algorithm (a definition: the tests emulate it): one-sided (Hestenes) complex Jacobi in float on A = H where
 * Nr >= Nt, else H^H (m x n, m = max(Nr, Nt)); never through the Gram matrix.  Column pairs (p, q), p < q, are rotated
 * in cyclic order and the rotations accumulated in an n x n unitary, so the short side's vectors are always a full
 * unitary matrix and the long side's the normalised columns of the rotated A.  With eps = max(m, n) 2^-23, a pair is
 * skipped where |a_p^H a_q| <= (eps / 2) |a_p| |a_q|, or where either column's squared norm is at or below eps^2 times
 * the largest column's squared norm at the start of the sweep (a rank-deficient channel, such as a LoS-only link, is
 * not rotated noise against noise).  A point is finished by the first sweep that rotates nothing; at most
 * HRT_SVD_MAX_SWEEPS (csrc/hrt_svd.h) sweeps are made, and a point that has rotated in all of them, or whose column
 * norms are not finite (NaN, Inf, or squares beyond float), reports HRT_SVD_NOT_CONVERGED and writes finite or NaN
 * values.  Order: sigma descending, equal values by their original column index, the vectors with them.  Column i is
 * null iff sigma_i <= eps sigma_0: its long-side vector is exact zeros (sigma_i is written as computed, the short side
 * stays unitary); H = 0 gives sigma = 0, the identity on the short side and zeros on the long side.  No gauge beyond
 * sigma real and >= 0 is fixed.  A point's bits depend on its own matrix only (not on its neighbours, the batch or
 * the launch); two calls give the same bytes.
 * hrt_compute_channel_svd traces and batches exactly as hrt_compute_array_channel does, keeps the accumulated H on the
 * device and decomposes once after the last batch (the SVD is not additive over batches); only the result is copied
 * back.  HRT_E_INVALID, before the device is touched: every refusal of hrt_compute_array_channel; a NULL out; every
 * refusal of hrt_channel_svd (include/hrt_device.h). */
#define HRT_SVD_U 1u
#define HRT_SVD_V 2u
#define HRT_SVD_NOT_CONVERGED 0xffffffffu
typedef struct {
    uint32_t num_rx, num_tx;                    /* receivers, transmitters */
    uint32_t nr, nt;                            /* the matrix of a point: Nr x Nt */
    uint32_t num_times, num_freqs;              /* T, K */
    uint32_t want;                              /* HRT_SVD_U | HRT_SVD_V (0: singular values only) */
} hrt_svd_spec;
uint64_t hrt_svd_out_bytes(const hrt_svd_spec *spec);   /* 0 for NULL */
int hrt_compute_channel_svd(Scene *scene, const Vec3 *rx_pos, const Vec3 *tx_pos, const Vec3 *rx_vel,
                            const Vec3 *tx_vel, float carrier_frequency_GHz, size_t num_rx, size_t num_tx,
                            size_t num_rays, size_t num_bounces, const hrt_channel_spec *spec,
                            const Vec3 *rx_elements, size_t num_rx_elements, const Vec3 *tx_elements,
                            size_t num_tx_elements, double array_frequency_hz, uint32_t want,
                            void *out /* host, hrt_svd_out_bytes bytes, layout above */, hrt_stats *stats);

/* Per-point linear MIMO equalizers (zero-forcing, LMMSE) of the array channel and their post-equalisation SINR, formed
 * on the device (include/hrt_device.h: hrt_channel_equalizer).  The model of a point -- one (rx, tx, pol, time,
 * frequency), H = H[rx][tx][:][:][pol][m][k] of hrt_compute_array_channel's layout, Nr x Nt -- is y = H x + n with
 * E[x x^H] = I and E[n n^H] = N0 I.  With lambda = N0 for HRT_EQ_LMMSE, lambda = 0 for HRT_EQ_ZF and
 * G = (H^H H + lambda I)^-1 (Nt x Nt), the outputs lie in one flat buffer of hrt_equalizer_out_bytes bytes, the point
 * axes innermost, the regions in this order (W is absent, size 0, without HRT_EQ_W in `flags`):
 *   W       complex [num_rx][num_tx][Nt][Nr][2][T][K]   W = G H^H: x_hat = W y                      (HRT_EQ_W)
 *   sinr    float   [num_rx][num_tx][Nt][2][T][K]       1 / (N0 G_ii) - [kind == HRT_EQ_LMMSE]: the noise enhancement
 *                                                       of ZF, the unbiased SINR of LMMSE, per stream i
 *   status  uint32  [num_rx][num_tx][2][T][K]           0, HRT_EQ_SINGULAR or HRT_EQ_NONFINITE
 * `noise` (N0) is one float per call, finite and > 0, for ZF too, where it only scales the SINR.  1 <= Nt <= 16,
 * 1 <= Nr <= 64; ZF requires Nr >= Nt, LMMSE accepts Nr < Nt.
 * Algorithm (a definition: the tests emulate it): modified Gram-Schmidt in float, column by column, on the augmented
 * matrix A = [H; sqrt(lambda) I] = Q R ((Nr + Nt) x Nt; just H for ZF), never through the Gram matrix.  The column
 * operations are carried on an Nt x Nt block T that starts as I and ends as R^-1; the bottom block of A is
 * sqrt(lambda) T throughout, so an inner product is the sum over H's rows plus lambda times the sum over T's.
 * G_ii is the squared norm of row i of T, and W^H = Q1 T^H with Q1 the top Nr rows of Q.  With u = (Nr + Nt) 2^-24, a
 * point is singular (HRT_EQ_SINGULAR) when a diagonal entry of R is at or below 2 u times the largest column norm of A
 * at the start; a point whose squared column norms do not sum to a finite float (NaN, Inf, or squares beyond float) is
 * HRT_EQ_NONFINITE, which takes precedence.  Either writes exact zeros to W and sinr, plus its status.  H = 0 under
 * LMMSE is regular (W = 0, sinr = 0, status 0); under ZF it is singular.  A point's bits depend on its own matrix only
 * (not on its neighbours, the batch or the launch); two calls give the same bytes.
 * Multi-user use: the transmitters of an uplink stacked along Nt, or the users of a downlink along Nr, in any tensor
 * of this layout, give the multi-user detector and the per-user SINR (hermespy_rt_amd.equalize.stack_users).
 * hrt_compute_channel_equalizer traces and batches exactly as hrt_compute_array_channel does, keeps the accumulated H
 * on the device and equalises once after the last batch: the equalizer is NOT additive over batches or shards (the
 * equalizer of a partial H is not the channel's), only the result is copied back.  HRT_E_INVALID, before the device is
 * touched: every refusal of hrt_compute_array_channel; a NULL out; every refusal of hrt_channel_equalizer
 * (include/hrt_device.h). */
#define HRT_EQ_ZF 0u
#define HRT_EQ_LMMSE 1u
#define HRT_EQ_W 1u
#define HRT_EQ_SINGULAR 1u
#define HRT_EQ_NONFINITE 2u
typedef struct {
    uint32_t num_rx, num_tx;                    /* receivers, transmitters */
    uint32_t nr, nt;                            /* the matrix of a point: Nr x Nt */
    uint32_t num_times, num_freqs;              /* T, K */
    uint32_t kind;                              /* HRT_EQ_ZF or HRT_EQ_LMMSE */
    uint32_t flags;                             /* HRT_EQ_W (0: sinr and status only) */
    float noise;                                /* N0, finite and > 0 */
} hrt_equalizer_spec;
uint64_t hrt_equalizer_out_bytes(const hrt_equalizer_spec *spec);   /* 0 for NULL */
int hrt_compute_channel_equalizer(Scene *scene, const Vec3 *rx_pos, const Vec3 *tx_pos, const Vec3 *rx_vel,
                                  const Vec3 *tx_vel, float carrier_frequency_GHz, size_t num_rx, size_t num_tx,
                                  size_t num_rays, size_t num_bounces, const hrt_channel_spec *spec,
                                  const Vec3 *rx_elements, size_t num_rx_elements, const Vec3 *tx_elements,
                                  size_t num_tx_elements, double array_frequency_hz, uint32_t kind, uint32_t flags,
                                  float noise,
                                  void *out /* host, hrt_equalizer_out_bytes bytes, layout above */, hrt_stats *stats);

/* Per-point linear MIMO precoders (maximum-ratio transmission, zero-forcing, regularised zero-forcing) of the array
 * channel and the downlink SINR of every stream behind them, formed on the device (include/hrt_device.h:
 * hrt_channel_precoder).  A point is one (rx, tx, pol, time, frequency) of a tensor of hrt_compute_array_channel's
 * layout: H = H[rx][tx][:][:][pol][m][k], Nr x Nt.  Row i of H is the channel to stream i, that is to user port i; Nt
 * is the number of transmit elements.  The model is y = H P s + n with E[s s^H] = I and E[n n^H] = N0 I.
 * Kinds (`kind`):
 *   HRT_PC_MRT   P0 = H^H
 *   HRT_PC_ZF    P0 = H^H (H H^H)^-1; needs Nr <= Nt
 *   HRT_PC_RZF   P0 = H^H (H H^H + alpha I)^-1 with `regularization` alpha, finite and > 0
 * Normalisation (`norm`), with `power` Ptot finite and > 0:
 *   HRT_PC_TOTAL   P = sqrt(Ptot / |P0|_F^2) P0
 *   HRT_PC_STREAM  column i of P is sqrt(Ptot / Nr) P0[:, i] / |P0[:, i]|
 * The outputs lie in one flat buffer of hrt_precoder_out_bytes bytes, the point axes innermost, the regions in this
 * order (P is absent, size 0, without HRT_PC_P in `flags`):
 *   P       complex [num_rx][num_tx][Nt][Nr][2][T][K]   the precoder: x = P s                              (HRT_PC_P)
 *   sinr    float   [num_rx][num_tx][Nr][2][T][K]       with E = H P, sinr_i = |E_ii|^2 / (sum_{j != i} |E_ij|^2 + N0)
 *   status  uint32  [num_rx][num_tx][2][T][K]           0, HRT_PC_SINGULAR or HRT_PC_NONFINITE
 * `noise` (N0), `power` and, for HRT_PC_RZF, `regularization` are one float each per call, finite and > 0 (the
 * regularization of the other kinds is not read).  1 <= Nr <= 16, 1 <= Nt <= 64, Nr * Nt * T * K <= 2^24, fewer than
 * 2^31 points.
 * Algorithm (a definition: the tests emulate it).  ZF and RZF: modified Gram-Schmidt in float, column by column, on the
 * augmented matrix A = [H^H; sqrt(alpha) I] = Q R ((Nt + Nr) x Nr; just H^H for ZF), never through the Gram matrix
 * H H^H: the equalizer's factorisation with the two sides swapped, the column operations carried on an Nr x Nr block T
 * that ends as R^-1, and P0 = Q1 T^H with Q1 the top Nt rows of Q.  The squared column norms of P0 are summed, P0 is
 * scaled by the rule of `norm`, and E = H P is formed from H itself and the scaled P that is stored, not from an identity
 * of the factorisation; the SINR is one float division.  With u = (Nr + Nt) 2^-24, a point is HRT_PC_SINGULAR when a
 * diagonal entry of R is at or below 2 u times the largest column norm of A at the start, or when a column of P0
 * (STREAM) or the whole P0 (TOTAL) has norm zero, as for H = 0 under every kind.  A point whose squared column norms of
 * A do not sum to a finite float (NaN, Inf, or squares beyond float) is HRT_PC_NONFINITE, which takes precedence; so
 * is a regular point whose squared norm of P0 is beyond float.  A flagged point writes exact zeros to P and sinr, plus
 * its status.  A point's bits depend on its own matrix only (not on its neighbours, the batch or the launch); two calls
 * give the same bytes.
 * Multi-user use: the users of a downlink stacked along Nr, in any tensor of this layout
 * (hermespy_rt_amd.equalize.stack_users(H, "rx")), give the base station's multi-user precoder and the SINR each user
 * sees.  hrt_compute_channel_precoder traces and batches exactly as hrt_compute_array_channel does, keeps the
 * accumulated H on the device and precodes once after the last batch: the precoder is NOT additive over batches or
 * shards (H is summed first), only the result is copied back.  HRT_E_INVALID, before the device is touched: every
 * refusal of hrt_compute_array_channel; a NULL out; every refusal of hrt_channel_precoder (include/hrt_device.h). */
#define HRT_PC_MRT 0u
#define HRT_PC_ZF 1u
#define HRT_PC_RZF 2u
#define HRT_PC_TOTAL 0u
#define HRT_PC_STREAM 1u
#define HRT_PC_P 1u
#define HRT_PC_SINGULAR 1u
#define HRT_PC_NONFINITE 2u
typedef struct {
    uint32_t num_rx, num_tx;                    /* receivers, transmitters */
    uint32_t nr, nt;                            /* the matrix of a point: Nr x Nt */
    uint32_t num_times, num_freqs;              /* T, K */
    uint32_t kind;                              /* HRT_PC_MRT, HRT_PC_ZF or HRT_PC_RZF */
    uint32_t norm;                              /* HRT_PC_TOTAL or HRT_PC_STREAM */
    uint32_t flags;                             /* HRT_PC_P (0: sinr and status only) */
    float noise;                                /* N0, finite and > 0 */
    float power;                                /* Ptot, finite and > 0 */
    float regularization;                       /* alpha, finite and > 0 (HRT_PC_RZF; not read otherwise) */
} hrt_precoder_spec;
uint64_t hrt_precoder_out_bytes(const hrt_precoder_spec *spec);   /* 0 for NULL */
int hrt_compute_channel_precoder(Scene *scene, const Vec3 *rx_pos, const Vec3 *tx_pos, const Vec3 *rx_vel,
                                 const Vec3 *tx_vel, float carrier_frequency_GHz, size_t num_rx, size_t num_tx,
                                 size_t num_rays, size_t num_bounces, const hrt_channel_spec *spec,
                                 const Vec3 *rx_elements, size_t num_rx_elements, const Vec3 *tx_elements,
                                 size_t num_tx_elements, double array_frequency_hz, uint32_t kind, uint32_t norm,
                                 uint32_t flags, float noise, float power, float regularization,
                                 void *out /* host, hrt_precoder_out_bytes bytes, layout above */, hrt_stats *stats);

/* Per-subband precoder codebook selection (limited feedback: the PMI search) on the array channel, formed on the device
 * (include/hrt_device.h: hrt_codebook_select).  A point is one (rx, tx, pol, time m, frequency k) of a tensor of
 * hrt_compute_array_channel's layout, H = H[rx][tx][:][:][pol][m][k], Nr x Nt.  A subband is `subband` = S consecutive
 * frequencies of one (rx, tx, pol, m); there are B = ceil(K / S) of them, the last holds the remainder, S = K is
 * wideband selection.  The codebook is complex [C][Nt][L], used as given (its power normalisation is the caller's).
 * For entry c at frequency k, E_c,k = H_k W_c is Nr x L, and with n the number of frequencies of the subband
 *   HRT_CS_POWER     mu_c = (1/n) sum_k |E_c,k|_F^2
 *   HRT_CS_CAPACITY  mu_c = (1/n) sum_k log2 det(I_L + E_c,k^H E_c,k / N0), `noise` N0 finite and > 0 (not read
 *                    under HRT_CS_POWER)
 * the sums over k ascending, and c* = argmax_c mu_c, the lowest index on a tie.
 * The outputs lie in one flat buffer of hrt_codebook_out_bytes bytes, the point axes innermost, in this order:
 *   index      uint32  [num_rx][num_tx][2][T][B]          c*
 *   metric     float   [num_rx][num_tx][2][T][B]          mu_c*
 *   status     uint32  [num_rx][num_tx][2][T][B]          0 or HRT_CS_NONFINITE
 *   table      float   [num_rx][num_tx][C][2][T][B]       every mu_c                                  (HRT_CS_TABLE)
 *   effective  complex [num_rx][num_tx][Nr][L][2][T][K]   E_c*,k: array_channel's layout with nt = L  (HRT_CS_EFFECTIVE)
 * `effective` holds the bits of the E that was scored, not a second evaluation in another order, and is taken as it is
 * by hrt_channel_equalizer, hrt_channel_svd and hrt_channel_precoder.
 * 1 <= Nr <= 16, 1 <= Nt <= 64, 1 <= L <= min(4, Nt), 1 <= C <= 4096, 1 <= S <= K, fewer than 2^31 points and fewer
 * than 2^31 table entries (num_rx num_tx C 2 T B).
 * Algorithm (a definition: the tests emulate it).  All float, no contraction.  Row i, layer l of E over t ascending
 * from zero, h = H[i][t], w = W[t][l]:  er = er + (hr wr - hi wi), ei = ei + (hr wi + hi wr).  Over the rows i
 * ascending, from zero: gd[a] = gd[a] + (er_a er_a + ei_a ei_a) and, for b < a (G = E^H E, lower triangle),
 * gr[a][b] = gr[a][b] + (er_a er_b + ei_a ei_b), gi[a][b] = gi[a][b] + (er_a ei_b - ei_a er_b).  POWER: the value of
 * a frequency is ((gd[0] + gd[1]) + gd[2]) + gd[3].  CAPACITY: A[a][a] = 1 + gd[a] / N0, A[a][b] = (gr / N0, gi / N0),
 * then the unpivoted LDL^H for j ascending: for m < j, v = A[j][m] less, for p < m ascending,
 * ((l_jp.r l_mp.r + l_jp.i l_mp.i) d_p, (l_jp.i l_mp.r - l_jp.r l_mp.i) d_p), and l_jm = (v.r / d_m, v.i / d_m);
 * d_j = A[j][j] less (l_jm.r l_jm.r + l_jm.i l_jm.i) d_m for m < j ascending; the determinant is ((d_0 d_1) d_2) d_3,
 * for L = 1 it is 1 + |E|^2 / N0, and the value is its log2 as csrc/hrt_codebook.h restates it in float operations
 * (exponent by the bits, a fixed polynomial on the mantissa; not the hardware's approximate instruction).  mu_c is the
 * sum of the values over k ascending, divided by (float)n.
 * A subband that holds a non-finite entry of H, or whose mu_c is not finite for some c (a square beyond float), is
 * HRT_CS_NONFINITE: index 0xFFFFFFFF, metric 0, zeros in its table row and in `effective` at all its frequencies.
 * H = 0 is regular: every mu_c ties and index 0 wins.  A subband's bytes depend on its own matrices and the codebook
 * only (not on neighbours, the tiling of the codebook or the launch); two calls give the same bytes; every output byte
 * is written exactly once.
 * hrt_compute_codebook_select traces and batches exactly as hrt_compute_array_channel does, keeps the accumulated H on
 * the device and selects once after the last batch: selection is NOT additive over batches or shards.  The codebook
 * is copied in, only the result is copied back.  HRT_E_INVALID, before the device is touched: every refusal of
 * hrt_compute_array_channel; a NULL codebook or out; every refusal of hrt_codebook_select (include/hrt_device.h). */
#define HRT_CS_POWER 0u
#define HRT_CS_CAPACITY 1u
#define HRT_CS_TABLE 1u
#define HRT_CS_EFFECTIVE 2u
#define HRT_CS_NONFINITE 1u
typedef struct {
    uint32_t num_rx, num_tx;                    /* receivers, transmitters */
    uint32_t nr, nt;                            /* the matrix of a point: Nr x Nt */
    uint32_t num_times, num_freqs;              /* T, K */
    uint32_t layers;                            /* L: columns of an entry, 1 .. min(4, Nt) */
    uint32_t entries;                           /* C: 1 .. 4096 */
    uint32_t subband;                           /* S: 1 .. K */
    uint32_t metric;                            /* HRT_CS_POWER or HRT_CS_CAPACITY */
    uint32_t flags;                             /* HRT_CS_TABLE | HRT_CS_EFFECTIVE */
    float noise;                                /* N0, finite and > 0 (HRT_CS_CAPACITY; not read otherwise) */
} hrt_codebook_spec;
uint64_t hrt_codebook_out_bytes(const hrt_codebook_spec *spec);   /* 0 for NULL */
int hrt_compute_codebook_select(Scene *scene, const Vec3 *rx_pos, const Vec3 *tx_pos, const Vec3 *rx_vel,
                                const Vec3 *tx_vel, float carrier_frequency_GHz, size_t num_rx, size_t num_tx,
                                size_t num_rays, size_t num_bounces, const hrt_channel_spec *spec,
                                const Vec3 *rx_elements, size_t num_rx_elements, const Vec3 *tx_elements,
                                size_t num_tx_elements, double array_frequency_hz,
                                const float *codebook /* host, complex [entries][Nt][layers] */, uint32_t layers,
                                uint32_t entries, uint32_t subband, uint32_t metric, uint32_t flags, float noise,
                                void *out /* host, hrt_codebook_out_bytes bytes, layout above */, hrt_stats *stats);

/* Per-point maximum-likelihood MIMO detection with max-log bit LLRs on the array channel, formed on the device
 * (include/hrt_device.h: hrt_channel_detect).  A point is one (rx, tx, pol, time m, frequency k).  H is
 * H[rx][tx][:][:][pol][m][k], Nr x Nt, from a tensor of hrt_compute_array_channel's layout; y is Y[rx][tx][:][pol][m][k]
 * from a tensor complex [num_rx][num_tx][Nr][2][T][K].  Nt is the number of streams.  The constellation is complex [M]
 * with M = 2^B, used as given (normalisation is the caller's); the index of a symbol is its bit label.  A hypothesis
 * q < Q = M^Nt assigns the symbol x_j = (q >> (j B)) & (M - 1) to stream j; bit b of stream j is
 * (x_j >> (B - 1 - b)) & 1, so b = 0 is the label's most significant bit, the first bit in the TS 38.211 order.
 * 1 <= Nr <= 64, 1 <= B <= 8, Nt B <= 12 (Q <= 4096, Nt <= 12), fewer than 2^31 points, the other size refusals are
 * hrt_channel_equalizer's; `noise` N0 finite and > 0.
 * Algorithm (a definition: the tests emulate it).  All float, no contraction.
 *   products   p_ij = H_ij s with s = S[x_j], as (hr sr - hi si, hr si + hi sr)
 *   row sums   e_i = (..((p_i0 + p_i1) + p_i2)..), over j ascending
 *   residuals  r_i = y_i - e_i
 *   distance   d_q = sum_i (r.re r.re + r.im r.im), over i ascending from zero
 *   decision   q* = argmin_q d_q, the lowest q on a tie
 *   minima     for every (j, b): m0 the minimum of d_q over the q whose bit is 0, m1 over those whose bit is 1
 *   LLR        llr[j][b] = (m0 - m1) / N0, one IEEE subtraction and one IEEE division: positive where bit 1 is the
 *              likelier
 * The outputs lie in one flat buffer of hrt_detect_out_bytes bytes, the point axes innermost, in this order:
 *   index   uint32  [num_rx][num_tx][2][T][K]           q*
 *   metric  float   [num_rx][num_tx][2][T][K]           d_q*
 *   status  uint32  [num_rx][num_tx][2][T][K]           0 or HRT_DT_NONFINITE
 *   llr     float   [num_rx][num_tx][Nt][B][2][T][K]    present only with HRT_DT_LLR in `flags`
 * A point is HRT_DT_NONFINITE when some d_q is not finite or, with HRT_DT_LLR, some LLR is not finite (a quotient
 * beyond float; without HRT_DT_LLR no LLR is formed and none is tested).  A non-finite entry of H or y reaches every
 * d_q; the flag is tracked explicitly, not left to a minimum that drops NaNs.  A flagged point writes index
 * 0xFFFFFFFF, metric 0 and zeros in its LLRs.  H = 0 is regular.  A point's bytes depend on its own H, y, the
 * constellation and N0 only; two calls give the same bytes; every output byte is written exactly once.
 * hrt_compute_channel_detect traces and batches exactly as hrt_compute_array_channel does, keeps the accumulated H on
 * the device, copies Y and the constellation up and detects once after the last batch: detection is NOT additive over
 * batches or shards.  Only the result is copied back.  HRT_E_INVALID, before the device is touched: every refusal of
 * hrt_compute_array_channel; a NULL Y, constellation or out; every refusal of hrt_channel_detect (include/hrt_device.h). */
#define HRT_DT_LLR 1u
#define HRT_DT_NONFINITE 1u
typedef struct {
    uint32_t num_rx, num_tx;                    /* receivers, transmitters */
    uint32_t nr, nt;                            /* the matrix of a point: Nr x Nt, Nt streams */
    uint32_t num_times, num_freqs;              /* T, K */
    uint32_t bits;                              /* B: bits per symbol, 1 .. 8, Nt B <= 12 */
    uint32_t flags;                             /* HRT_DT_LLR */
    float noise;                                /* N0, finite and > 0 */
} hrt_detect_spec;
uint64_t hrt_detect_out_bytes(const hrt_detect_spec *spec);   /* 0 for NULL */
int hrt_compute_channel_detect(Scene *scene, const Vec3 *rx_pos, const Vec3 *tx_pos, const Vec3 *rx_vel,
                               const Vec3 *tx_vel, float carrier_frequency_GHz, size_t num_rx, size_t num_tx,
                               size_t num_rays, size_t num_bounces, const hrt_channel_spec *spec,
                               const Vec3 *rx_elements, size_t num_rx_elements, const Vec3 *tx_elements,
                               size_t num_tx_elements, double array_frequency_hz,
                               const float *Y /* host, complex [num_rx][num_tx][Nr][2][T][K] */,
                               const float *constellation /* host, complex [2^bits] */, uint32_t bits, uint32_t flags,
                               float noise, void *out /* host, hrt_detect_out_bytes bytes, layout above */,
                               hrt_stats *stats);

/* Per-point K-best tree-search MIMO detection with list max-log bit LLRs on the array channel, formed on the device
 * (include/hrt_device.h: hrt_channel_kbest): near-ML detection beyond hrt_detect_spec's Q <= 4096.  Points, H, y, the
 * constellation, the digits x_j of a hypothesis q and the bits are hrt_detect_spec's.  1 <= Nr <= 64 (Nr < Nt is
 * accepted), 1 <= Nt <= 16, 1 <= B <= 8, Nt B <= 32, the list size K in {1, 2, 4, 8, 16, 32, 64}, `noise` N0 and
 * `clip` finite and > 0, the size refusals of hrt_channel_detect.
 * Algorithm (a definition: the tests emulate it).  All float, no contraction.  An inner product <a, c> = a^H c or a
 * squared norm of columns is summed in the order csrc/hrt_kbest.h fixes (per lane over its rows ascending, then a
 * butterfly over the hrt_kbest_form(Nr, Nt, K) lanes of the point); its terms are (ar cr + ai ci), (ar ci - ai cr),
 * (ar ar + ai ai).
 *   start      A = [H | y], Nr x (Nt + 1).  n_c the squared norms of its columns; thr = ((float)(Nr + Nt) 2^-23)
 *              sqrtf(largest n_c of H's columns); the sum of all n_c, over c ascending, not finite: NONFINITE.
 *   position t = 0 .. Nt - 1:
 *     pick       without HRT_KB_SORTED the stream c = t.  With it (sorted QR), of the streams not yet picked the one
 *                with the smallest squared norm of its current residual column, recomputed from the column (not
 *                downdated), the lowest stream on a tie (a strict < over the streams ascending).
 *     diagonal   r = sqrtf(that squared norm).  !(r > thr): a NULL column -- row t of R is 0, z_t = 0, no column
 *                changes, the point is HRT_KB_DEFICIENT.  Else R_tt = r (real) and a_c <- a_c / r, entry by entry.
 *     project    for every stream u not yet picked, ascending, then for y: w = <a_c, a_u>, R_tu = w (z_t = w for y),
 *                a_u <- a_u - w a_c as (ur - (wr cr - wi ci), ui - (wr ci + wi cr)).
 *   rho        the squared norm of what is left of the column y.  Not finite: NONFINITE.
 *   tree       the list starts as one empty path with PED = rho and key 0.  For position i = Nt - 1 down to 0, with c
 *              the stream at position i, every path of the list forms
 *                b = z_i - (..((R_i,i+1 s_i+1) + R_i,i+2 s_i+2) + ..), positions ascending, s_t the path's symbol
 *                    of the stream at position t, products (rr sr - ri si, rr si + ri sr); b = z_i at i = Nt - 1
 *              and M children, x = 0 .. M - 1 with s = S[x]:
 *                e = (b.re - R_ii s.re, b.im - R_ii s.im),  PED' = PED + (e.re e.re + e.im e.im),
 *                key' = key | x << (c B)
 *              (a PED' that is not finite: NONFINITE).  Of all children of the level the K with the smallest PED'
 *              make the next list, the lower key on equal PED'.  A key holds every decided stream's digit at its OWN
 *              position j B (not the detection position's) and zeros elsewhere, so keys are distinct, the list is
 *              defined independently of how it is found, and a leaf's key is its hypothesis q.
 *   decision   index: the leaf of the final list with the smallest PED, the lowest q on a tie; metric: its PED.  The
 *              PED of a leaf is |y - H s(q)|^2 up to rounding (rho included), comparable with hrt_detect_spec's d_q.
 *   LLR        for every (j, b): m0 the minimum PED over the FINAL list's leaves whose bit is 0, m1 over those whose
 *              bit is 1 (not over every leaf visited).  Both exist: v = (m0 - m1) / N0 (not finite: NONFINITE), then
 *              v > clip: clip, v < -clip: -clip.  No leaf with bit 0 (the decision's bit is 1): +clip; none with
 *              bit 1: -clip.
 * With K = 1 and HRT_KB_SORTED this is ordered successive interference cancellation.  Where M^(Nt-1) <= K no path is
 * ever pruned before the last level, so index and metric are the exhaustive minimum of the PED; where M^Nt <= K the
 * LLRs are the exhaustive ones, clamped.
 * The outputs lie in one flat buffer of hrt_kbest_out_bytes bytes, in hrt_detect_spec's order and shapes: index
 * uint32, metric float, status uint32 [num_rx][num_tx][2][T][K], llr float [num_rx][num_tx][Nt][B][2][T][K] (present
 * only with HRT_KB_LLR).  status is 0, HRT_KB_NONFINITE (1) or HRT_KB_DEFICIENT (2): a NONFINITE point writes status 1
 * exactly, index 0xFFFFFFFF, metric 0 and zeros in its LLRs (with Nt B = 32 that index is also a valid hypothesis:
 * status decides).  The LLR quotient is tested only with HRT_KB_LLR.  A non-finite entry of H or y reaches a column
 * norm; the flag is tracked explicitly.  A DEFICIENT point is detected all the same: a null level ties all its children
 * and the lower keys survive.  H = 0 follows the same rules: every column is null (status 2), index 0, metric |y|^2.
 * A point's bytes depend on its own H, y, the constellation, N0, K, clip and flags only; two calls give the same
 * bytes; every output byte is written exactly once.
 * hrt_compute_channel_kbest traces and batches exactly as hrt_compute_channel_detect does and detects once after the
 * last batch: detection is NOT additive over batches or shards.  HRT_E_INVALID, before the device is touched: every
 * refusal of hrt_compute_array_channel; a NULL Y, constellation or out; every refusal of hrt_channel_kbest. */
#define HRT_KB_LLR 1u
#define HRT_KB_SORTED 2u
#define HRT_KB_NONFINITE 1u
#define HRT_KB_DEFICIENT 2u
typedef struct {
    uint32_t num_rx, num_tx;                    /* receivers, transmitters */
    uint32_t nr, nt;                            /* the matrix of a point: Nr x Nt, Nt streams */
    uint32_t num_times, num_freqs;              /* T, K */
    uint32_t bits;                              /* B: bits per symbol, 1 .. 8, Nt B <= 32 */
    uint32_t flags;                             /* HRT_KB_LLR | HRT_KB_SORTED */
    uint32_t k;                                 /* the list size: 1, 2, 4, .. 64 */
    float noise;                                /* N0, finite and > 0 */
    float clip;                                 /* the LLR clip, finite and > 0 */
} hrt_kbest_spec;
uint64_t hrt_kbest_out_bytes(const hrt_kbest_spec *spec);   /* 0 for NULL */
int hrt_compute_channel_kbest(Scene *scene, const Vec3 *rx_pos, const Vec3 *tx_pos, const Vec3 *rx_vel,
                              const Vec3 *tx_vel, float carrier_frequency_GHz, size_t num_rx, size_t num_tx,
                              size_t num_rays, size_t num_bounces, const hrt_channel_spec *spec,
                              const Vec3 *rx_elements, size_t num_rx_elements, const Vec3 *tx_elements,
                              size_t num_tx_elements, double array_frequency_hz,
                              const float *Y /* host, complex [num_rx][num_tx][Nr][2][T][K] */,
                              const float *constellation /* host, complex [2^bits] */, uint32_t bits, uint32_t flags,
                              uint32_t k, float noise, float clip,
                              void *out /* host, hrt_kbest_out_bytes bytes, layout above */, hrt_stats *stats);

/* Per-link power statistics of the traced paths, formed on the device (include/hrt_device.h: hrt_power_profiles).
 * INCOHERENT sums over the terms hrt_channel sums (the same parts; blocked records add nothing and are not counted):
 *   LoS entry (shard rank 0, LoS not blocked): coincident a = 1, tau = nu = 0, u_rx = (1, 0, 0), u_tx = (-1, 0, 0);
 *     clear a = HRT_LOS_A (TE = TM), tau = HRT_LOS_TAU, nu = HRT_LOS_FS, u_tx = HRT_LOS_DIR, u_rx = -u_tx;
 *   scatter record: a = a_te / a_tm, tau, nu = the float difference FS0 - DFS (the path list's freq_shift),
 *     u_rx = directions_rx, u_tx = the launch direction of the record's ray (as hrt_compute_array_channel).
 * For pol 0 = TE, 1 = TM, p = |a^pol|^2 in FP64; every sum is FP64.  With L = num_rx * num_tx links, `out` holds
 * four regions in this order (a region switched off is absent):
 *   moments   [L][2][HRT_POWER_FIELDS]: COUNT (terms summed), P = sum p, P_TAU = sum p tau, P_TAU2 = sum p tau^2,
 *             P_NU = sum p nu, P_NU2 = sum p nu^2, P_URX_X/Y/Z = sum p u_rx, P_UTX_X/Y/Z = sum p u_tx, P_LOS (the
 *             LoS term's p);
 *   pdp       [L][2][Ld]: bin i = floor((double(tau) - tau0) / dtau) (IEEE double division) gets p when
 *             0 <= i < Ld; terms outside the window stay in the moments;
 *   arrival   [L][2][Nth][Nph] and departure [L][2][Nth][Nph]: p by the direction of u_rx / u_tx, zenith
 *             theta = acos(clamp(u_z, -1, 1)), bin min(floor(theta / pi * Nth), Nth - 1); azimuth
 *             phi = atan2(u_y, u_x), bin floor((phi + pi) / (2 pi) * Nph), index Nph wrapping to 0.
 * Ld = 0: no pdp; Nth = Nph = 0: no angular spectra.  Everything is additive: shards and batches add up to the whole.
 * The histograms are formed in fixed point, rint(p 2^(62 - E)) with 2^E >= 2 P of the call: a bin is within
 * N 2^-61 P of the FP64 sum of its N terms.  hrt_power_out_doubles gives the size of `out` (0 for a NULL spec).
 * hrt_compute_power_profiles traces and batches like hrt_compute_channel (one device, one download at the end).
 * HRT_E_INVALID, before the device is touched: parts 0 or with unknown bits; Ld > 2^16; tau0 or dtau not finite or
 * dtau <= 0 when Ld > 0; exactly one of Nth, Nph 0; Nth * Nph > 2^14; num_rx * num_tx > 65535;
 * num_rx * num_tx * (Ld + 2 Nth Nph) > 2^26. */
enum {
    HRT_POWER_COUNT = 0, HRT_POWER_P, HRT_POWER_P_TAU, HRT_POWER_P_TAU2, HRT_POWER_P_NU, HRT_POWER_P_NU2,
    HRT_POWER_P_URX_X, HRT_POWER_P_URX_Y, HRT_POWER_P_URX_Z, HRT_POWER_P_UTX_X, HRT_POWER_P_UTX_Y, HRT_POWER_P_UTX_Z,
    HRT_POWER_P_LOS,
    HRT_POWER_FIELDS
};
typedef struct {
    double tau0_s, dtau_s;                      /* delay bin i: [tau0 + i dtau, tau0 + (i + 1) dtau) */
    uint32_t num_delay_bins;                    /* Ld */
    uint32_t num_zenith_bins, num_azimuth_bins; /* Nth, Nph */
    uint32_t parts;                             /* HRT_CHANNEL_LOS | HRT_CHANNEL_SCATTER */
} hrt_power_spec;
uint64_t hrt_power_out_doubles(size_t num_rx, size_t num_tx, const hrt_power_spec *spec);
int hrt_compute_power_profiles(Scene *scene, const Vec3 *rx_pos, const Vec3 *tx_pos, const Vec3 *rx_vel,
                               const Vec3 *tx_vel, float carrier_frequency_GHz, size_t num_rx, size_t num_tx,
                               size_t num_rays, size_t num_bounces, const hrt_power_spec *spec,
                               double *out /* hrt_power_out_doubles, layout above */, hrt_stats *stats);

/* Per-link spatial covariance matrices of an antenna array, formed on the device (include/hrt_device.h:
 * hrt_array_covariance): the second-order statistics of hrt_compute_array_channel's H under independent uniform path
 * phases.  For every link, polarisation pol (0 = TE, 1 = TM) and element pair of ONE side:
 *     R_rx[rx][tx][pol][i][i'] = sum_p |a_p^pol|^2 s_i(u_p^rx) conj(s_i'(u_p^rx)),   s_i(u) = exp(j 2 pi f_a r_i . u / c)
 *     R_tx[rx][tx][pol][j][j'] = sum_p |a_p^pol|^2 t_j(u_p^tx) conj(t_j'(u_p^tx)),   t_j(u) = exp(j 2 pi f_a q_j . u / c)
 * so that R_rx = E[H H^H] / Nt and R_tx[j][j'] = E[sum_i H[i][j] conj(H[i][j'])] / Nr.
 *   Terms: those of hrt_compute_power_profiles (the same `parts`): the LoS entry, added by shard rank 0 only where
 *     the LoS is not blocked (coincident a = 1, u_rx = (1, 0, 0), u_tx = (-1, 0, 0); clear a = HRT_LOS_A,
 *     u_tx = HRT_LOS_DIR, u_rx = -u_tx), and every unblocked scatter record of every bounce; blocked records add nothing.
 *   Directions: u_rx = directions_rx of the record, u_tx = the launch direction of the record's global path (as
 *     hrt_compute_array_channel).
 *   Weight: p = |a^pol|^2, the exact FP64 value of the float amplitudes rounded once to float.
 *   Steering: exactly the array families' rule: the phase in revolutions is (f_a / c) (r . u) in FP64 from float
 *     operands, reduced to its fraction and evaluated in float (sincospi), once per (term, element) and never per
 *     element pair; the products and sums are float (one f32 MFMA per record, tile and polarisation).
 *   Hermitian to the bit: only the upper triangle (i' >= i) is summed; R[i'][i] is written as its conjugate and the
 *     diagonal with imaginary part exactly 0.
 *   Additive: shards and batches add up to the whole; record chunks are added in a fixed order without atomics, so two
 *     calls with the same inputs give the same bits.
 * Elements and f_a are hrt_compute_array_channel's; `sides` selects R_rx (HRT_COV_RX), R_tx (HRT_COV_TX) or both.  A
 * side that is not asked for needs no elements (its count and pointer are ignored) and writes nothing.
 * out: one flat complex buffer, re/im interleaved floats (numpy complex64): R_rx [num_rx][num_tx][2][Nr][Nr], then
 * R_tx [num_rx][num_tx][2][Nt][Nt]; an absent side has size 0.  hrt_covariance_out_floats (include/hrt_device.h, beside
 * hrt_array_spec) gives its size in floats.  hrt_compute_array_covariance traces and batches like hrt_compute_channel
 * (one device, one download at the end).  HRT_E_INVALID, before the device is touched: NULL spec; parts 0 or with
 * unknown bits; sides 0 or with unknown bits; a requested side with 0 or more than 256 elements or a NULL element
 * pointer; an offset or f_a not finite; f_a <= 0; num_rx * num_tx > 65535; num_rx * num_tx * 2 * (Nr^2 + Nt^2) > 2^26. */
#define HRT_COV_RX 1u
#define HRT_COV_TX 2u
typedef struct {
    uint32_t parts;                             /* HRT_CHANNEL_LOS | HRT_CHANNEL_SCATTER */
    uint32_t sides;                             /* HRT_COV_RX | HRT_COV_TX */
} hrt_covariance_spec;
int hrt_compute_array_covariance(Scene *scene, const Vec3 *rx_pos, const Vec3 *tx_pos, const Vec3 *rx_vel,
                                 const Vec3 *tx_vel, float carrier_frequency_GHz, size_t num_rx, size_t num_tx,
                                 size_t num_rays, size_t num_bounces, const hrt_covariance_spec *spec,
                                 const Vec3 *rx_elements, size_t num_rx_elements, const Vec3 *tx_elements,
                                 size_t num_tx_elements, double array_frequency_hz,
                                 float *out /* complex interleaved, layout above */, hrt_stats *stats);

/* The K strongest paths of every link, selected on the device (include/hrt_device.h: hrt_dominant_paths): the short
 * list of (gain, delay, Doppler, arrival and departure direction) a link-level simulator builds a sparse channel
 * from, instead of the full path list.  The ELIGIBLE terms of a link are exactly the terms hrt_channel sums (the same
 * `parts`): the LoS entry (shard rank 0, LoS not blocked) and every unblocked scatter record of every bounce; blocked
 * records are not eligible and are not counted.  The ranking quantity is the FP64 value
 *     power = ((double)te_re*te_re + (double)te_im*te_im) + ((double)tm_re*tm_re + (double)tm_im*tm_im)
 * of the float amplitudes (every product exact, denormal amplitudes kept; the LoS entry has a_te = a_tm = (a, 0)).
 * Term A precedes term B if power_A > power_B, or the powers are equal and bounce_A < bounce_B, or powers and bounces
 * are equal and path_A < path_B; bounce is -1 for the LoS entry and path is the GLOBAL path index (the one
 * hrt_compute_paths_list reports), so within a link the order is strict and does not depend on shards, batches or
 * the order the device visits the records in.
 * A kept term is a record of 72 bytes.  Its float fields are bit for bit the floats the other families sum:
 * freq_shift the float difference FS0 - DFS, u_rx the record's directions_rx, u_tx the launch direction of the
 * record's ray; the LoS entry has u_tx = HRT_LOS_DIR and u_rx = -u_tx (the sign bit of every component flipped), a
 * coincident one a = 1, tau = freq_shift = 0, u_tx = (-1, 0, 0), u_rx = (1, -0, -0).  `tri` is the triangle the ray left towards the RX: here the flat index in
 * the reference's (mesh, face) loop order (in the device-resident entry: the row of the device table, see
 * hrt_device.h).
 * out: hrt_dominant_out_bytes bytes (0 for a NULL or refused spec): a header uint64_t [L][2] = {kept, eligible} per
 * link (L = num_rx * num_tx), then hrt_dominant_path [L][K], K = max_paths.  Within a link the first
 * kept = min(K, eligible) slots are the first `kept` eligible terms in the order above and the remaining slots are
 * all-zero bytes: the whole buffer is a function of the inputs.
 * hrt_compute_dominant_paths traces and batches like hrt_compute_channel (one device, one download at the end; the
 * batches are merged on the device).  HRT_E_INVALID, before the device is touched: NULL spec; max_paths 0 or > 1024;
 * parts 0 or with unknown bits; num_rx * num_tx > 65535; num_rx * num_tx * max_paths > 2^22. */
typedef struct {
    double power;
    uint64_t path;            /* global path; LoS: UINT64_MAX */
    int32_t bounce;           /* LoS: -1 */
    uint32_t tri;             /* LoS: UINT32_MAX */
    float a_te_re, a_te_im, a_tm_re, a_tm_im, tau, freq_shift;
    float u_rx[3], u_tx[3];
} hrt_dominant_path;
typedef struct {
    uint32_t max_paths;                         /* K */
    uint32_t parts;                             /* HRT_CHANNEL_LOS | HRT_CHANNEL_SCATTER */
} hrt_dominant_spec;
uint64_t hrt_dominant_out_bytes(size_t num_rx, size_t num_tx, const hrt_dominant_spec *spec);
int hrt_compute_dominant_paths(Scene *scene, const Vec3 *rx_pos, const Vec3 *tx_pos, const Vec3 *rx_vel,
                               const Vec3 *tx_vel, float carrier_frequency_GHz, size_t num_rx, size_t num_tx,
                               size_t num_rays, size_t num_bounces, const hrt_dominant_spec *spec,
                               void *out /* hrt_dominant_out_bytes, layout above */, hrt_stats *stats);

/* The antenna-array channel of dominant-path lists, formed on the device (include/hrt_device.h:
 * hrt_sparse_array_channel): the second half of the sentence above, the sparse channel built from the short lists and
 * evaluated again for any grid, array or time axis, without the workspace.  The input is a buffer in exactly the layout
 * hrt_dominant_paths writes: a header uint64_t [L][2] = {kept, eligible}, then hrt_dominant_path [L][K], L = num_rx *
 * num_tx, K = max_paths.  For every link, element pair (i, j), polarisation (0 = TE, 1 = TM), time sample m and
 * frequency k:
 *     n = min(kept[link], K)
 *     H[rx][tx][i][j][pol][m][k] = sum over slots p < n of
 *           a_p^pol exp(j 2 pi (nu_p t_m - f_k tau_p)) exp(j 2 pi f_a (r_i . u_rx_p + q_j . u_tx_p) / c)
 * a^TE = (a_te_re, a_te_im), a^TM = (a_tm_re, a_tm_im); tau, nu = freq_shift, u_rx and u_tx are the slot's floats; f_k,
 * t_m, f_a, c, the element offsets and the output layout are hrt_compute_array_channel's:
 * out: complex [num_rx][num_tx][Nr][Nt][2][num_times][num_freqs], re/im interleaved (numpy complex64).
 * The LoS entry is an ordinary slot (bounce -1) without a rule of its own.  power, path, bounce and tri are not read.
 * Slots at or beyond n are never read: whatever they hold does not reach the output.  A link with n = 0 writes zeros
 * (or leaves `out` unchanged when accumulating).  With Nr = Nt = 1 and zero offsets this is the SISO channel of the
 * list.  Where kept = eligible for a link the result is hrt_compute_array_channel's for the same parts, up to the
 * order of the float32 sums; where kept < eligible it is the channel of the strongest K terms.
 * Every byte of `out` is written exactly once (added to once when accumulating); no atomics and no scratch buffer; two
 * calls with the same input give the same bytes; a link's bytes depend only on its own slots, the grid and the
 * elements; a non-finite field in one link's list stays within that link's outputs.
 * hrt_compute_sparse_array_channel runs hrt_compute_dominant_paths' batch loop (the lists merged on the device) and
 * evaluates the merged lists once after the last batch; only `out`, and the lists if paths_out is not NULL
 * (hrt_dominant_out_bytes, `tri` as hrt_compute_dominant_paths reports it), is copied back.  HRT_E_INVALID, before the
 * device is touched: every hrt_compute_dominant_paths check; every grid check of hrt_channel_spec (the spec's parts
 * are not read: the parts are the dominant spec's); Nr or Nt outside 1..1024; Nr * Nt * num_times * num_freqs > 2^24;
 * an offset or f_a not finite; f_a <= 0. */
typedef struct {
    double f0_hz, df_hz;  uint32_t num_freqs;   /* f_k = f0 + k*df */
    double t0_s, dt_s;    uint32_t num_times;   /* t_m = t0 + m*dt */
    uint32_t num_rx, num_tx;                    /* L = num_rx * num_tx links */
    uint32_t max_paths;                         /* K: slots per link */
} hrt_sparse_spec;
int hrt_compute_sparse_array_channel(Scene *scene, const Vec3 *rx_pos, const Vec3 *tx_pos, const Vec3 *rx_vel,
                                     const Vec3 *tx_vel, float carrier_frequency_GHz, size_t num_rx, size_t num_tx,
                                     size_t num_rays, size_t num_bounces, const hrt_dominant_spec *dominant_spec,
                                     const hrt_channel_spec *grid, const Vec3 *rx_elements, size_t num_rx_elements,
                                     const Vec3 *tx_elements, size_t num_tx_elements, double array_frequency_hz,
                                     float *out /* complex interleaved, layout above */,
                                     void *paths_out /* hrt_dominant_out_bytes, or NULL */, hrt_stats *stats);

/* The beamformed channel of dominant-path lists, formed on the device (include/hrt_device.h:
 * hrt_sparse_beam_channel): what hrt_compute_beam_channel gives from the workspace, here from a buffer in exactly the
 * layout hrt_dominant_paths writes (header uint64_t [L][2] = {kept, eligible}, then hrt_dominant_path [L][K]), so that
 * a beam sweep, a codebook search or a re-evaluation on another grid or time axis costs what the list costs.  For every
 * link, RX beam a, TX beam b, polarisation, time sample m and frequency k:
 *     n = min(kept[link], K)
 *     B[rx][tx][a][b][pol][m][k] = sum over slots p < n of
 *           a_p^pol exp(j 2 pi (nu_p t_m - f_k tau_p)) g_rx[a](u_rx_p) g_tx[b](u_tx_p)
 *     g_rx[a](u) = sum_i conj(W_rx[a][i]) exp(j 2 pi f_a r_i . u / c),   g_tx[b](u) = sum_j W_tx[b][j] exp(j 2 pi f_a q_j . u / c)
 * The grid, the element offsets and f_a are hrt_compute_array_channel's; the weight layout and conventions are
 * hrt_compute_beam_channel's: rx_weights complex [Br][Nr], tx_weights complex [Bt][Nt], re/im interleaved, the RX
 * codebook applied conjugated, nothing normalised, one codebook for all RX and one for all TX.
 * out: complex [num_rx][num_tx][Br][Bt][2][num_times][num_freqs], re/im interleaved (numpy complex64).
 * The slot rules are hrt_compute_sparse_array_channel's: the LoS entry is an ordinary slot; power, path, bounce and tri
 * are not read; slots at or beyond n are never read; a link with n = 0 writes zeros (or leaves `out` unchanged when
 * accumulating).  Where kept = eligible for a link the result is hrt_compute_beam_channel's for the same parts, up to
 * the order of the float32 sums; it equals hrt_compute_sparse_array_channel's H contracted with the two codebooks
 * wherever H can be formed, and H is never formed: there is no limit on Nr * Nt.  Every byte of `out` is written
 * exactly once (added to once when accumulating); no atomics and no scratch buffer; two calls with the same input give
 * the same bytes; a link's bytes depend only on its own slots below n, the grid, the elements and the weights.
 * hrt_compute_sparse_beam_channel runs hrt_compute_dominant_paths' batch loop (the lists merged on the device) and
 * evaluates the merged lists once after the last batch; only `out`, and the lists if paths_out is not NULL, is copied
 * back.  HRT_E_INVALID, before the device is touched: every hrt_compute_dominant_paths check; every grid check of
 * hrt_channel_spec (the grid's parts are not read: the parts are the dominant spec's); Nr or Nt outside 1..256; Br or
 * Bt outside 1..256; Br * Bt * num_times * num_freqs > 2^24; an offset, a weight or f_a not finite; f_a <= 0. */
int hrt_compute_sparse_beam_channel(Scene *scene, const Vec3 *rx_pos, const Vec3 *tx_pos, const Vec3 *rx_vel,
                                    const Vec3 *tx_vel, float carrier_frequency_GHz, size_t num_rx, size_t num_tx,
                                    size_t num_rays, size_t num_bounces, const hrt_dominant_spec *dominant_spec,
                                    const hrt_channel_spec *grid, const Vec3 *rx_elements, size_t num_rx_elements,
                                    const Vec3 *tx_elements, size_t num_tx_elements, double array_frequency_hz,
                                    const float *rx_weights /* complex [Br][Nr] */, size_t num_rx_beams,
                                    const float *tx_weights /* complex [Bt][Nt] */, size_t num_tx_beams,
                                    float *out /* complex interleaved, layout above */,
                                    void *paths_out /* hrt_dominant_out_bytes, or NULL */, hrt_stats *stats);

/* The antenna-array impulse responses of dominant-path lists, formed on the device (include/hrt_device.h:
 * hrt_sparse_array_taps): the time-domain half of the above, what hrt_compute_array_taps gives from the workspace, here
 * from a buffer in exactly the layout hrt_dominant_paths writes (header uint64_t [L][2] = {kept, eligible}, then
 * hrt_dominant_path [L][K]).  An inverse FFT of hrt_compute_sparse_array_channel is no substitute: it aliases every
 * delay beyond 1 / df.  For every link, element pair (i, j), polarisation, time sample m and tap l_i = l_min + i:
 *     n = min(kept[link], K)
 *     h[rx][tx][i][j][pol][m][l] = sum over slots p < n of
 *           a_p^pol exp(j 2 pi (nu_p t_m - f_c tau_p)) exp(j 2 pi f_a (r_i . u_rx_p + q_j . u_tx_p) / c)
 *           sinc(l_min + l - f_s tau_p)
 * with hrt_taps_spec's t_m, l_i, f_s, f_c and sinc rule, and hrt_compute_array_taps' element offsets, f_a and layout:
 * out: complex [num_rx][num_tx][Nr][Nt][2][num_times][num_taps], re/im interleaved (numpy complex64).
 * The slot rules are hrt_compute_sparse_array_channel's: the LoS entry is an ordinary slot; power, path, bounce and tri
 * are not read; slots at or beyond n are never read; a link with n = 0 writes zeros (or leaves `out` unchanged when
 * accumulating).  Where kept = eligible for a link the result is hrt_compute_array_taps' for the same parts, up to the
 * order of the float32 sums.  Every byte of `out` is written exactly once (added to once when accumulating); no atomics
 * and no scratch buffer; two calls with the same input give the same bytes; a link's bytes depend only on its own slots
 * below n, the grid and the elements.
 * hrt_compute_sparse_array_taps runs hrt_compute_dominant_paths' batch loop (the lists merged on the device) and
 * evaluates the merged lists once after the last batch; only `out`, and the lists if paths_out is not NULL, is copied
 * back.  HRT_E_INVALID, before the device is touched: every hrt_compute_dominant_paths check; every grid check of
 * hrt_taps_spec (the grid's parts are not read: the parts are the dominant spec's); Nr or Nt outside 1..1024; Nr * Nt *
 * num_times * num_taps > 2^24; an offset or f_a not finite; f_a <= 0. */
typedef struct {
    double fs_hz, fc_hz;                        /* sampling rate, baseband centre frequency */
    double t0_s, dt_s;                          /* t_m = t0 + m*dt */
    int32_t l_min;  uint32_t num_taps;          /* l_i = l_min + i */
    uint32_t num_times;
    uint32_t num_rx, num_tx;                    /* L = num_rx * num_tx links */
    uint32_t max_paths;                         /* K: slots per link */
} hrt_sparse_taps_spec;
int hrt_compute_sparse_array_taps(Scene *scene, const Vec3 *rx_pos, const Vec3 *tx_pos, const Vec3 *rx_vel,
                                  const Vec3 *tx_vel, float carrier_frequency_GHz, size_t num_rx, size_t num_tx,
                                  size_t num_rays, size_t num_bounces, const hrt_dominant_spec *dominant_spec,
                                  const hrt_taps_spec *grid, const Vec3 *rx_elements, size_t num_rx_elements,
                                  const Vec3 *tx_elements, size_t num_tx_elements, double array_frequency_hz,
                                  float *out /* complex interleaved, layout above */,
                                  void *paths_out /* hrt_dominant_out_bytes, or NULL */, hrt_stats *stats);

/* The beamformed impulse responses of dominant-path lists, formed on the device (include/hrt_device.h:
 * hrt_sparse_beam_taps): what hrt_compute_beam_taps gives from the workspace, here from a buffer in exactly the layout
 * hrt_dominant_paths writes (header uint64_t [L][2] = {kept, eligible}, then hrt_dominant_path [L][K]), so that a beam
 * sweep in the time domain, or a re-evaluation at another rate, tap window, codebook or time axis, costs what the list
 * costs.  An inverse FFT of hrt_compute_sparse_beam_channel is no substitute: it aliases every delay beyond 1 / df.
 * For every link, RX beam a, TX beam b, polarisation, time sample m and tap l_i = l_min + i:
 *     n = min(kept[link], K)
 *     h[rx][tx][a][b][pol][m][l] = sum over slots p < n of
 *           a_p^pol exp(j 2 pi (nu_p t_m - f_c tau_p)) g_rx[a](u_rx_p) g_tx[b](u_tx_p) sinc(l_min + l - f_s tau_p)
 *     g_rx[a](u) = sum_i conj(W_rx[a][i]) exp(j 2 pi f_a r_i . u / c),   g_tx[b](u) = sum_j W_tx[b][j] exp(j 2 pi f_a q_j . u / c)
 * with hrt_taps_spec's t_m, l_i, f_s, f_c and sinc rule, hrt_compute_array_taps' element offsets and f_a, and
 * hrt_compute_beam_taps' weight layout and conventions: rx_weights complex [Br][Nr], tx_weights complex [Bt][Nt],
 * re/im interleaved, the RX codebook applied conjugated, nothing normalised, one codebook for all RX and one for all TX.
 * out: complex [num_rx][num_tx][Br][Bt][2][num_times][num_taps], re/im interleaved (numpy complex64).
 * The slot rules are hrt_compute_sparse_array_channel's: the LoS entry is an ordinary slot; power, path, bounce and tri
 * are not read; slots at or beyond n are never read; a link with n = 0 writes zeros (or leaves `out` unchanged when
 * accumulating).  Where kept = eligible for a link the result is hrt_compute_beam_taps' for the same parts, up to the
 * order of the float32 sums; it equals hrt_compute_sparse_array_taps' h contracted with the two codebooks wherever h
 * can be formed, and h is never formed: there is no limit on Nr * Nt.  Every byte of `out` is written exactly once
 * (added to once when accumulating); no atomics and no scratch buffer; two calls with the same input give the same
 * bytes; a link's bytes depend only on its own slots below n, the grid, the elements and the weights.
 * hrt_compute_sparse_beam_taps runs hrt_compute_dominant_paths' batch loop (the lists merged on the device) and
 * evaluates the merged lists once after the last batch; only `out`, and the lists if paths_out is not NULL, is copied
 * back.  HRT_E_INVALID, before the device is touched: every hrt_compute_dominant_paths check; every grid check of
 * hrt_taps_spec (the grid's parts are not read: the parts are the dominant spec's); Nr or Nt outside 1..256; Br or Bt
 * outside 1..256; Br * Bt * num_times * num_taps > 2^24; an offset, a weight or f_a not finite; f_a <= 0. */
int hrt_compute_sparse_beam_taps(Scene *scene, const Vec3 *rx_pos, const Vec3 *tx_pos, const Vec3 *rx_vel,
                                 const Vec3 *tx_vel, float carrier_frequency_GHz, size_t num_rx, size_t num_tx,
                                 size_t num_rays, size_t num_bounces, const hrt_dominant_spec *dominant_spec,
                                 const hrt_taps_spec *grid, const Vec3 *rx_elements, size_t num_rx_elements,
                                 const Vec3 *tx_elements, size_t num_tx_elements, double array_frequency_hz,
                                 const float *rx_weights /* complex [Br][Nr] */, size_t num_rx_beams,
                                 const float *tx_weights /* complex [Bt][Nt] */, size_t num_tx_beams,
                                 float *out /* complex interleaved, layout above */,
                                 void *paths_out /* hrt_dominant_out_bytes, or NULL */, hrt_stats *stats);

/* Antenna radiation patterns and orientations (include/hrt_device.h: hrt_apply_patterns; csrc/hrt_patterns.hip).  A
 * pattern is a real factor per (path, RX, TX): for every unblocked scatter record p of link (rx, tx), and for every
 * clear LoS entry,
 *     w_p = fl32( F_rx(R_rx[rx] u_p^rx) F_tx(R_tx[tx] u_p^tx) ),     a_te, a_tm <- fl32(field * w_p)
 * for each of the four float amplitude fields (LoS: HRT_LOS_A).  u_p^rx and u_p^tx are the directions the steering
 * terms of the array families use, both outward look directions from their endpoint: u^rx = directions_rx of the
 * record, u^tx = the launch direction of the record's global path; LoS: u^tx = HRT_LOS_DIR, u^rx = -u^tx.  R is the
 * 3 x 3 row-major world -> local rotation of the endpoint (NULL: identity).  In the local frame the boresight is +x,
 * the zenith theta = atan2(hypot(x, y), z) is measured from +z and the azimuth is phi = atan2(y, x); R u is not
 * re-normalised (both angles are scale-invariant).  F >= 0 is a linear FIELD amplitude (sqrt of the gain), one
 * pattern per side shared by all endpoints of that side, g = 10^(gain_db / 20) (formed in double, passed as float):
 *   HRT_PATTERN_ISOTROPIC  F = g
 *   HRT_PATTERN_DIPOLE     a half-wave dipole along local z: F = g sqrt(1.64) cos((pi / 2) cos theta) / sin theta;
 *                          where sin theta < 2^-12 its limit F = g sqrt(1.64) (pi / 4) sin theta
 *   HRT_PATTERN_TR38901    TR 38.901 table 7.3-1: A_v = -min(12 ((theta_deg - 90) / 65)^2, 30),
 *                          A_h = -min(12 (phi_deg / 65)^2, 30), A = -min(-(A_v + A_h), 30), F = g 10^((8 + A) / 20)
 *   HRT_PATTERN_TABLE      float amplitudes [num_zenith][num_azimuth] at theta_i = pi i / (num_zenith - 1)
 *                          (2 <= num_zenith <= 181) and phi_k = -pi + 2 pi k / num_azimuth, periodic
 *                          (1 <= num_azimuth <= 360), bilinear; every one-dimensional interpolation is
 *                          v0 + s (v1 - v0), so a constant table returns its constant exactly
 * Untouched, bit for bit: blocked records (their direction fields are not read), the slots from a block's count up to
 * cap, mask words, hit blocks, the tau, DFS and direction fields, blocked LoS entries, and COINCIDENT LoS entries
 * (status 0): their amplitude is 1 by definition, never read from the workspace, so a coincident link is not weighted.
 *
 * hrt_compute_set_patterns sets the patterns the path-sum drop-ins of the calling thread apply (hrt_compute_channel,
 * _array_channel, _taps, _array_taps, _beam_channel, _beam_taps, _power_profiles, _dominant_paths, _array_covariance,
 * _received_signal): after each batch's trace and before its sums.  The pointer is kept, not the contents: what it
 * points to must stay valid until it is cleared (NULL), and is read once at the entry of each call.  compute_paths,
 * hrt_compute_paths_ex / _interleaved / _list and the export path never see it.  Tables and rotations are HOST arrays
 * here; rx_rot [num_rx][9] / tx_rot [num_tx][9] may be NULL (identity).  A drop-in call refuses (HRT_E_INVALID) what
 * hrt_apply_patterns refuses, a table value that is not finite or < 0, and a rotation count that is not the call's
 * num_rx / num_tx. */
#define HRT_PATTERN_ISOTROPIC 0u
#define HRT_PATTERN_DIPOLE 1u
#define HRT_PATTERN_TR38901 2u
#define HRT_PATTERN_TABLE 3u
typedef struct {
    uint32_t kind, num_zenith, num_azimuth;     /* HRT_PATTERN_*; the table's nodes (HRT_PATTERN_TABLE only) */
    float gain_db;
    const float *d_table;                       /* [num_zenith][num_azimuth] (HRT_PATTERN_TABLE only) */
} hrt_pattern;
typedef struct {
    hrt_pattern rx, tx;                         /* d_table: HOST memory here */
    const float *rx_rot, *tx_rot;               /* host [num_rx][9], [num_tx][9]; NULL: identity */
    size_t num_rx, num_tx;                      /* the rotation counts (of a non-NULL rotation array) */
} hrt_patterns_host;
void hrt_compute_set_patterns(const hrt_patterns_host *patterns);

/* Human-readable description of the last error on this thread ("" if none). */
const char *hrt_last_error(void);

/* "hermespy-rt_amd <version> (gfx950)" */
const char *hrt_version(void);

/* Between calls compute_paths keeps: (with HRT_HOST_LAUNCH=1) the launch-direction table and launch
 * order of the last num_rays; the device workspace and page-locked staging of the last call; and
 * the calling thread's helper threads of the dense writer, parked (csrc/host/compute_paths.c).
 * This releases all three.  Environment: HRT_NO_CACHE=1 keeps no buffers. */
void hrt_cache_clear(void);

#ifdef __cplusplus
}
#endif
#endif /* HERMESPY_RT_H */
