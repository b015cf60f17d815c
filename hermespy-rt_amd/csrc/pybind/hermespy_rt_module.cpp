// hermespy_rt -- Python surface of the compute_paths hot path (pybind11).
//
// Same module name, function signature, keyword names and ChannelInfo attributes as the
// reference's binding (compute_paths_pybind11.cpp:99-210), so `import hermespy_rt` /
// `from .rt import compute_paths` users switch by putting this module on the path:
//
//   compute_paths(mesh_filepath, rx_positions, tx_positions, rx_velocities, tx_velocities,
//                 carrier_frequency, num_rx, num_tx, num_paths, num_bounces)
//       -> (los: ChannelInfo, scatter: ChannelInfo)
//   ChannelInfo.num_paths                  int   (1 / num_bounces*num_paths)
//   ChannelInfo.directions_rx/_tx          float32  (num_rx, num_tx, num_paths, 3)
//   ChannelInfo.a_te / a_tm                complex64 (num_rx, num_tx, num_paths)
//   ChannelInfo.tau / freq_shift           float32  (num_rx, num_tx, num_paths)
// The scatter path axis is bounce*num_paths + path.
//
// Deliberate differences from the reference binding (its defects):
//   * C linkage is declared on every platform (the reference only does under _WIN32 and
//     fails to import on Linux);
//   * slots the tracer does not write (dead rays, blocked records' directions, the scatter
//     directions_tx) read 0 instead of uninitialised heap memory;
//   * the RaysInfo buffers the reference allocates (too small, Q13) and then throws away are
//     not produced at all;
//   * an unreadable scene file raises ValueError instead of exit(8); tracer errors raise
//     RuntimeError; the GIL is released while the GPU works;
//   * the complex amplitudes are written in place (hrt_compute_paths_interleaved) and the arrays
//     start as untouched zero pages: the reference's binding fills four planes and interleaves them
//     afterwards (:44-97) -- on C3 those passes were 0.45 s around a 0.04 s call.
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>

#include <complex>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <stdexcept>
#include <algorithm>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include <sys/mman.h>

#include "hermespy_rt.h"

namespace py = pybind11;

namespace {

using farr = py::array_t<float, py::array::c_style | py::array::forcecast>;

struct ChannelInfoPy {
    size_t num_paths = 0;
    py::array_t<float> directions_rx, directions_tx;
    py::array_t<std::complex<float>> a_te, a_tm;
    py::array_t<float> tau, freq_shift;
};

const Vec3 *as_vec3(const farr &a, size_t n, const char *name)
{
    if ((size_t)a.size() != 3 * n)
        throw std::invalid_argument(std::string(name) + ": expected " + std::to_string(n) +
                                    " x 3 values");
    return reinterpret_cast<const Vec3 *>(a.data());
}

// Output arrays are fresh zero pages behind a capsule -- calloc() for small ones, an anonymous mapping
// advised to use huge pages for big ones (C3: 2.3 GB): "reads 0 where the reference writes nothing"
// then costs no pass over the memory, the pages are first touched by the threads of the dense writer
// that fill them, and with 2 MiB pages those first touches are ~10^3 faults instead of ~6 10^5
// (py::array_t + memset was 0.3 s of a 0.5 s call on C3).
struct Mapping { void *p; size_t bytes; };
template <typename T>
py::array_t<T> zeros(std::vector<size_t> shape)
{
    size_t n = 1;
    for (size_t d : shape) n *= d;
    const size_t bytes = (n ? n : 1) * sizeof(T);
    if (bytes >= ((size_t)4 << 20)) {
        const size_t huge = (size_t)2 << 20, len = (bytes + huge - 1) & ~(huge - 1);
        void *p = mmap(nullptr, len, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
        if (p == MAP_FAILED) throw std::bad_alloc();
        (void)madvise(p, len, MADV_HUGEPAGE);   // a hint; plain pages are as correct
        py::capsule owner(new Mapping{p, len}, [](void *q) {
            Mapping *m = static_cast<Mapping *>(q);
            munmap(m->p, m->bytes);
            delete m;
        });
        return py::array_t<T>(shape, static_cast<T *>(p), owner);
    }
    T *p = static_cast<T *>(std::calloc(n ? n : 1, sizeof(T)));
    if (!p) throw std::bad_alloc();
    py::capsule owner(p, [](void *q) { std::free(q); });
    return py::array_t<T>(shape, p, owner);
}

void check_scene_file(const std::string &path)
{
    FILE *f = std::fopen(path.c_str(), "rb");
    if (!f) throw py::value_error("cannot open scene file: " + path);
    char magic[3] = {0, 0, 0};
    const size_t got = std::fread(magic, 1, 3, f);
    std::fclose(f);
    if (got != 3 || std::memcmp(magic, "HRT", 3) != 0)
        throw py::value_error("not an HRT scene file: " + path);
}

// one channel block: every output is written in place by the library -- the complex amplitudes too,
// through hrt_compute_paths_interleaved (re at [2 i], im at [2 i + 1] of the complex64 arrays)
struct ChannelBuffers {
    ChannelInfoPy out;
    ChannelInfo c{};
    ChannelBuffers(size_t nrx, size_t ntx, size_t n)
    {
        out.num_paths = n;
        out.directions_rx = zeros<float>({nrx, ntx, n, 3});
        out.directions_tx = zeros<float>({nrx, ntx, n, 3});
        out.a_te = zeros<std::complex<float>>({nrx, ntx, n});
        out.a_tm = zeros<std::complex<float>>({nrx, ntx, n});
        out.tau = zeros<float>({nrx, ntx, n});
        out.freq_shift = zeros<float>({nrx, ntx, n});
        c.num_rays = (uint32_t)n;
        c.directions_rx = reinterpret_cast<Vec3 *>(out.directions_rx.mutable_data());
        c.directions_tx = reinterpret_cast<Vec3 *>(out.directions_tx.mutable_data());
        float *te = reinterpret_cast<float *>(out.a_te.mutable_data());
        float *tm = reinterpret_cast<float *>(out.a_tm.mutable_data());
        c.a_te_re = te; c.a_te_im = te + 1;
        c.a_tm_re = tm; c.a_tm_im = tm + 1;
        c.tau = out.tau.mutable_data();
        c.freq_shift = out.freq_shift.mutable_data();
    }
};

std::tuple<ChannelInfoPy, ChannelInfoPy> compute_paths_py(
    const std::string &mesh_filepath, farr rx_positions, farr tx_positions, farr rx_velocities,
    farr tx_velocities, float carrier_frequency, unsigned long num_rx, unsigned long num_tx,
    unsigned long num_paths, unsigned long num_bounces)
{
    if (!num_rx || !num_tx || !num_paths || !num_bounces)
        throw std::invalid_argument("num_rx, num_tx, num_paths, num_bounces must be > 0");
    const Vec3 *rxp = as_vec3(rx_positions, num_rx, "rx_positions");
    const Vec3 *txp = as_vec3(tx_positions, num_tx, "tx_positions");
    const Vec3 *rxv = as_vec3(rx_velocities, num_rx, "rx_velocities");
    const Vec3 *txv = as_vec3(tx_velocities, num_tx, "tx_velocities");
    check_scene_file(mesh_filepath);

    ChannelBuffers los(num_rx, num_tx, 1), scat(num_rx, num_tx, num_bounces * num_paths);
    int rc;
    std::string err;
    {
        py::gil_scoped_release nogil;
        Scene scene = scene_load(mesh_filepath.c_str());
        rc = hrt_compute_paths_interleaved(&scene, rxp, txp, rxv, txv, carrier_frequency, num_rx, num_tx,
                                           num_paths, num_bounces, &los.c, nullptr, &scat.c, nullptr,
                                           nullptr);
        if (rc != HRT_OK) err = hrt_last_error();
        free_scene(&scene);
    }
    if (rc != HRT_OK)
        throw std::runtime_error("hermespy_rt.compute_paths failed (" + std::to_string(rc) +
                                 "): " + err);
    return {std::move(los.out), std::move(scat.out)};
}

// compute_paths_list: the same call with the result as ONE list of path records (extension; the
// reference has no such form).  Returns a dict of numpy arrays, entry n being the record the dense
// form holds at [rx[n], tx[n], bounce[n] * num_paths + path[n]].
template <typename T>
py::array_t<T> copy_out(const T *src, std::vector<size_t> shape)
{
    py::array_t<T> a(shape);
    if (a.size()) std::memcpy(a.mutable_data(), src, sizeof(T) * (size_t)a.size());
    return a;
}

py::dict compute_paths_list_py(const std::string &mesh_filepath, farr rx_positions, farr tx_positions,
                               farr rx_velocities, farr tx_velocities, float carrier_frequency,
                               unsigned long num_rx, unsigned long num_tx, unsigned long num_paths,
                               unsigned long num_bounces, bool include_blocked)
{
    if (!num_rx || !num_tx || !num_paths || !num_bounces)
        throw std::invalid_argument("num_rx, num_tx, num_paths, num_bounces must be > 0");
    const Vec3 *rxp = as_vec3(rx_positions, num_rx, "rx_positions");
    const Vec3 *txp = as_vec3(tx_positions, num_tx, "tx_positions");
    const Vec3 *rxv = as_vec3(rx_velocities, num_rx, "rx_velocities");
    const Vec3 *txv = as_vec3(tx_velocities, num_tx, "tx_velocities");
    check_scene_file(mesh_filepath);
    // the list stays where the library built it: every numpy array is a view of one of its fields
    // and keeps it alive through one shared capsule (copying 1.3 GB of fields was 0.19 s of a
    // 0.24 s call on C3); only the complex amplitudes are formed here, from the re/im planes
    hrt_path_list *plp = new hrt_path_list;
    std::memset(plp, 0, sizeof *plp);
    py::capsule owner(plp, [](void *q) {
        hrt_path_list *p = static_cast<hrt_path_list *>(q);
        hrt_path_list_free(p);
        delete p;
    });
    hrt_path_list &pl = *plp;
    int rc;
    std::string err;
    {
        py::gil_scoped_release nogil;
        Scene scene = scene_load(mesh_filepath.c_str());
        rc = hrt_compute_paths_list(&scene, rxp, txp, rxv, txv, carrier_frequency, num_rx, num_tx,
                                    num_paths, num_bounces, include_blocked ? 1 : 0, &pl, nullptr);
        if (rc != HRT_OK) err = hrt_last_error();
        free_scene(&scene);
    }
    if (rc != HRT_OK)
        throw std::runtime_error("hermespy_rt.compute_paths_list failed (" + std::to_string(rc) +
                                 "): " + err);
    const size_t n = (size_t)pl.num;
    py::array_t<std::complex<float>> te = zeros<std::complex<float>>({n}), tm = zeros<std::complex<float>>({n});
    {
        py::gil_scoped_release nogil;
        std::complex<float> *pte = te.mutable_data(), *ptm = tm.mutable_data();
        const unsigned nt = (unsigned)std::max<size_t>(1, std::min<size_t>(8, n / 1000000));
        std::vector<std::thread> th;
        auto part = [&](size_t i0, size_t i1) {
            for (size_t i = i0; i < i1; ++i) {
                pte[i] = {pl.a_te_re[i], pl.a_te_im[i]};
                ptm[i] = {pl.a_tm_re[i], pl.a_tm_im[i]};
            }
        };
        for (unsigned k = 1; k < nt; ++k) th.emplace_back(part, n * k / nt, n * (k + 1) / nt);
        part(0, n / nt);
        for (auto &x : th) x.join();
    }
    auto view = [&](auto *ptr, std::vector<size_t> shape) {
        using T = std::remove_cv_t<std::remove_pointer_t<decltype(ptr)>>;
        return py::array_t<T>(shape, ptr, owner);
    };
    py::dict d;
    d["rx"] = view(pl.rx, {n});
    d["tx"] = view(pl.tx, {n});
    d["bounce"] = view(pl.bounce, {n});
    d["path"] = view(pl.path, {n});
    d["a_te"] = te;
    d["a_tm"] = tm;
    d["tau"] = view(pl.tau, {n});
    d["direction_rx"] = view(reinterpret_cast<float *>(pl.direction_rx), {n, 3});
    d["freq_shift"] = view(pl.freq_shift, {n});
    d["unblocked"] = view(reinterpret_cast<bool *>(pl.unblocked), {n});
    d["mesh"] = view(pl.mesh, {n});
    d["face"] = view(pl.face, {n});
    d["los"] = view(pl.los, {(size_t)num_rx, (size_t)num_tx, (size_t)8});
    return d;
}

// What the nine path-sum entries (compute_channel, compute_array_channel, compute_taps, compute_array_taps,
// compute_power_profiles, compute_dominant_paths, compute_beam_channel, compute_beam_taps, compute_array_covariance) and compute_received_signal share.  The counts and the four position / velocity arguments, checked ...
struct endpoints {
    const Vec3 *rxp, *txp, *rxv, *txv;
    endpoints(const farr &rx_positions, const farr &tx_positions, const farr &rx_velocities,
              const farr &tx_velocities, unsigned long num_rx, unsigned long num_tx, unsigned long num_paths,
              unsigned long num_bounces)
    {
        if (!num_rx || !num_tx || !num_paths || !num_bounces)
            throw std::invalid_argument("num_rx, num_tx, num_paths, num_bounces must be > 0");
        rxp = as_vec3(rx_positions, num_rx, "rx_positions");
        txp = as_vec3(tx_positions, num_tx, "tx_positions");
        rxv = as_vec3(rx_velocities, num_rx, "rx_velocities");
        txv = as_vec3(tx_velocities, num_tx, "tx_velocities");
    }
};

// ... the element arguments of the two array entries, and whether Nr * Nt * grid points are within the library's
// limits (an output it would refuse is not allocated), the `parts` word ...
struct array_elements {
    const Vec3 *rxe, *txe;
    size_t nr, nt;
    array_elements(const farr &rx_elements, const farr &tx_elements)
        : rxe(reinterpret_cast<const Vec3 *>(rx_elements.data())),
          txe(reinterpret_cast<const Vec3 *>(tx_elements.data())), nr((size_t)rx_elements.size() / 3),
          nt((size_t)tx_elements.size() / 3)
    {
        if (rx_elements.size() % 3 || tx_elements.size() % 3)
            throw std::invalid_argument("rx_elements and tx_elements must have shape (n, 3)");
    }
    bool fits(unsigned long long grid) const
    {
        const unsigned long long pts = (unsigned long long)nr * nt * grid;
        return pts > 0 && pts <= (1ull << 24) && nr <= 1024 && nt <= 1024;
    }
};

uint32_t parts_word(bool los, bool scatter)
{
    return (los ? HRT_CHANNEL_LOS : 0u) | (scatter ? HRT_CHANNEL_SCATTER : 0u);
}

// ... the `patterns` keyword: None, or a dict with rx and tx (pattern dicts of hermespy_rt_amd.patterns: kind, gain_db,
// table; None: isotropic) and rx_orientation and tx_orientation ((n, 3, 3) world -> local rotations, or one (3, 3) for
// all endpoints of the side; None: identity).  A scope guard: the patterns are set for this thread's path-sum call while
// it lives and cleared when it goes (hrt_compute_set_patterns); the library checks the contents when the call starts ...
struct pattern_scope {
    hrt_patterns_host host{};
    farr tables[2];
    std::vector<float> rot[2];
    bool set = false;

    static void pattern(const py::object &o, const char *side, hrt_pattern &f, farr &keep)
    {
        if (o.is_none()) return;   // isotropic, 0 dB
        if (!py::isinstance<py::dict>(o))
            throw py::value_error(std::string("patterns['") + side + "'] must be a pattern dict (kind, gain_db, table)");
        const py::dict d = o.cast<py::dict>();
        if (!d.contains("kind") || !d.contains("gain_db"))
            throw py::value_error(std::string("patterns['") + side + "'] needs kind and gain_db");
        const long long kind = d["kind"].cast<long long>();
        if (kind < 0 || kind > 0xffffffffLL)
            throw py::value_error(std::string("patterns['") + side + "']: kind must fit 32 bits");
        f.kind = (uint32_t)kind;
        f.gain_db = d["gain_db"].cast<float>();
        if (d.contains("table") && !d["table"].is_none()) {
            keep = d["table"].cast<farr>();
            if (keep.ndim() != 2)
                throw py::value_error(std::string("patterns['") + side + "']: the table must have shape (num_zenith, num_azimuth)");
            f.num_zenith = (uint32_t)keep.shape(0);
            f.num_azimuth = (uint32_t)keep.shape(1);
            f.d_table = keep.data();
        }
    }

    static const float *rotations(const py::object &o, const char *name, size_t n, std::vector<float> &keep, size_t &count)
    {
        if (o.is_none()) return nullptr;
        const farr a = o.cast<farr>();
        const bool one = a.ndim() == 2 && a.shape(0) == 3 && a.shape(1) == 3;
        if (!one && !(a.ndim() == 3 && a.shape(1) == 3 && a.shape(2) == 3))
            throw py::value_error(std::string("patterns['") + name + "'] must have shape (3, 3) or (n, 3, 3)");
        count = one ? n : (size_t)a.shape(0);
        keep.resize(9u * count);
        for (size_t i = 0; i < keep.size(); ++i) keep[i] = a.data()[one ? i % 9u : i];
        return keep.data();
    }

    pattern_scope(const py::object &patterns, size_t num_rx, size_t num_tx)
    {
        if (patterns.is_none()) return;
        if (!py::isinstance<py::dict>(patterns))
            throw py::value_error("patterns must be None or a dict (rx, tx, rx_orientation, tx_orientation)");
        const py::dict d = patterns.cast<py::dict>();
        for (auto kv : d) {
            const std::string k = py::str(kv.first);
            if (k != "rx" && k != "tx" && k != "rx_orientation" && k != "tx_orientation")
                throw py::value_error("patterns: unknown key '" + k + "' (rx, tx, rx_orientation, tx_orientation)");
        }
        auto get = [&](const char *k) { return d.contains(k) ? py::object(d[k]) : py::object(py::none()); };
        pattern(get("rx"), "rx", host.rx, tables[0]);
        pattern(get("tx"), "tx", host.tx, tables[1]);
        host.rx_rot = rotations(get("rx_orientation"), "rx_orientation", num_rx, rot[0], host.num_rx);
        host.tx_rot = rotations(get("tx_orientation"), "tx_orientation", num_tx, rot[1], host.num_tx);
        hrt_compute_set_patterns(&host);
        set = true;
    }
    ~pattern_scope()
    {
        if (set) hrt_compute_set_patterns(nullptr);
    }
    pattern_scope(const pattern_scope &) = delete;
    pattern_scope &operator=(const pattern_scope &) = delete;
};

// ... and the call of the entry (`name`): the scene loaded and freed around `call` without the GIL; a refused argument raises ValueError, any other error RuntimeError
template <typename F>
void run_pathsum(const char *name, const std::string &mesh_filepath, F call)
{
    int rc;
    std::string err;
    {
        py::gil_scoped_release nogil;
        Scene scene = scene_load(mesh_filepath.c_str());
        rc = call(&scene);
        if (rc != HRT_OK) err = hrt_last_error();
        free_scene(&scene);
    }
    if (rc == HRT_E_INVALID) throw py::value_error(std::string("hermespy_rt.") + name + ": " + err);
    if (rc != HRT_OK)
        throw std::runtime_error(std::string("hermespy_rt.") + name + " failed (" + std::to_string(rc) + "): " + err);
}

// compute_channel: the channel frequency response of the traced paths, formed on the device (extension; see
// hrt_compute_channel in hermespy_rt.h): complex64 (num_rx, num_tx, 2, num_times, num_freqs), pol 0 = TE, 1 = TM,
// H = sum_p a_p exp(j 2 pi (nu_p t_m - f_k tau_p)) with f_k = f0 + k df ABSOLUTE (Hz), t_m = t0 + m dt (s).
py::array_t<std::complex<float>> compute_channel_py(
    const std::string &mesh_filepath, farr rx_positions, farr tx_positions, farr rx_velocities, farr tx_velocities,
    float carrier_frequency, unsigned long num_rx, unsigned long num_tx, unsigned long num_paths,
    unsigned long num_bounces, double f0, double df, unsigned long num_freqs, double t0, double dt,
    unsigned long num_times, bool los, bool scatter,
    py::object patterns)
{
    const endpoints e(rx_positions, tx_positions, rx_velocities, tx_velocities, num_rx, num_tx, num_paths, num_bounces);
    if (num_freqs > 0xffffffffUL || num_times > 0xffffffffUL)
        throw std::invalid_argument("num_freqs and num_times must fit 32 bits");
    check_scene_file(mesh_filepath);
    hrt_channel_spec spec{};
    spec.f0_hz = f0; spec.df_hz = df; spec.num_freqs = (uint32_t)num_freqs;
    spec.t0_s = t0; spec.dt_s = dt; spec.num_times = (uint32_t)num_times;
    spec.parts = parts_word(los, scatter);
    // (the library validates the spec before it traces anything: a refused one raises ValueError)
    py::array_t<std::complex<float>> out({(size_t)num_rx, (size_t)num_tx, (size_t)2, (size_t)num_times,
                                          (size_t)num_freqs});
    float *dst = reinterpret_cast<float *>(out.mutable_data());
    const pattern_scope pattern_guard(patterns, num_rx, num_tx);
    run_pathsum("compute_channel", mesh_filepath, [&](Scene *scene) {
        return hrt_compute_channel(scene, e.rxp, e.txp, e.rxv, e.txv, carrier_frequency, num_rx, num_tx, num_paths,
                                   num_bounces, &spec, dst, nullptr);
    });
    return out;
}

// compute_array_channel: the antenna-array channel of the traced paths, formed on the device (extension; see
// hrt_compute_array_channel in hermespy_rt.h): complex64 (num_rx, num_tx, Nr, Nt, 2, num_times, num_freqs).  Element
// offsets are (Nr, 3) / (Nt, 3) metres from the traced RX / TX positions; array_frequency (Hz) defaults to the carrier.
py::array_t<std::complex<float>> compute_array_channel_py(
    const std::string &mesh_filepath, farr rx_positions, farr tx_positions, farr rx_velocities, farr tx_velocities,
    float carrier_frequency, unsigned long num_rx, unsigned long num_tx, unsigned long num_paths,
    unsigned long num_bounces, double f0, double df, unsigned long num_freqs, farr rx_elements, farr tx_elements,
    double t0, double dt, unsigned long num_times, bool los, bool scatter, py::object array_frequency,
    py::object patterns)
{
    const endpoints e(rx_positions, tx_positions, rx_velocities, tx_velocities, num_rx, num_tx, num_paths, num_bounces);
    if (num_freqs > 0xffffffffUL || num_times > 0xffffffffUL)
        throw std::invalid_argument("num_freqs and num_times must fit 32 bits");
    const array_elements a(rx_elements, tx_elements);
    const double fa = array_frequency.is_none() ? (double)carrier_frequency * 1e9 : array_frequency.cast<double>();
    check_scene_file(mesh_filepath);
    hrt_channel_spec spec{};
    spec.f0_hz = f0; spec.df_hz = df; spec.num_freqs = (uint32_t)num_freqs;
    spec.t0_s = t0; spec.dt_s = dt; spec.num_times = (uint32_t)num_times;
    spec.parts = parts_word(los, scatter);
    // (the library validates everything before it traces anything: a refused call raises ValueError.  An output
    // beyond the 2^24 points of the limit would be refused, so only one within it is allocated.)
    const bool fits = a.fits((unsigned long long)num_times * num_freqs);
    py::array_t<std::complex<float>> out(fits ? std::vector<size_t>{(size_t)num_rx, (size_t)num_tx, a.nr, a.nt, (size_t)2,
                                                                    (size_t)num_times, (size_t)num_freqs}
                                              : std::vector<size_t>{1});
    float *dst = reinterpret_cast<float *>(out.mutable_data());
    const pattern_scope pattern_guard(patterns, num_rx, num_tx);
    run_pathsum("compute_array_channel", mesh_filepath, [&](Scene *scene) {
        return hrt_compute_array_channel(scene, e.rxp, e.txp, e.rxv, e.txv, carrier_frequency, num_rx, num_tx, num_paths,
                                         num_bounces, &spec, a.rxe, a.nr, a.txe, a.nt, fa, dst, nullptr);
    });
    return out;
}

// compute_channel_svd: the per-point MIMO SVD of compute_array_channel's H, formed on the device (extension; see
// hrt_compute_channel_svd in hermespy_rt.h): a dict of views of one buffer -- sigma float32 (num_rx, num_tx, n, 2,
// num_times, num_freqs) with n = min(Nr, Nt); u complex64 (num_rx, num_tx, Nr, n, 2, num_times, num_freqs) and v
// (num_rx, num_tx, Nt, n, ...), both None with vectors=False; sweeps uint32 (num_rx, num_tx, 2, num_times, num_freqs)
// -- and the buffer itself (uint8).
py::dict compute_channel_svd_py(
    const std::string &mesh_filepath, farr rx_positions, farr tx_positions, farr rx_velocities, farr tx_velocities,
    float carrier_frequency, unsigned long num_rx, unsigned long num_tx, unsigned long num_paths,
    unsigned long num_bounces, double f0, double df, unsigned long num_freqs, farr rx_elements, farr tx_elements,
    double t0, double dt, unsigned long num_times, bool los, bool scatter, py::object array_frequency, bool vectors,
    py::object patterns)
{
    const endpoints e(rx_positions, tx_positions, rx_velocities, tx_velocities, num_rx, num_tx, num_paths, num_bounces);
    if (num_freqs > 0xffffffffUL || num_times > 0xffffffffUL || num_rx > 0xffffffffUL || num_tx > 0xffffffffUL)
        throw std::invalid_argument("num_rx, num_tx, num_freqs and num_times must fit 32 bits");
    const array_elements a(rx_elements, tx_elements);
    const double fa = array_frequency.is_none() ? (double)carrier_frequency * 1e9 : array_frequency.cast<double>();
    check_scene_file(mesh_filepath);
    hrt_channel_spec spec{};
    spec.f0_hz = f0; spec.df_hz = df; spec.num_freqs = (uint32_t)num_freqs;
    spec.t0_s = t0; spec.dt_s = dt; spec.num_times = (uint32_t)num_times;
    spec.parts = parts_word(los, scatter);
    const uint32_t want = vectors ? (HRT_SVD_U | HRT_SVD_V) : 0u;
    // (the library validates everything before it traces anything: a refused call raises ValueError; an output beyond
    // its limits is not allocated)
    const size_t nr = a.nr, nt = a.nt, n = nr < nt ? nr : nt, big = nr < nt ? nt : nr;
    const size_t pts = (size_t)num_rx * num_tx * 2u * num_times * num_freqs;
    const bool fits = a.fits((unsigned long long)num_times * num_freqs) && n <= 16u && big <= 64u && pts < (1ull << 31);
    hrt_svd_spec sv{};
    sv.num_rx = (uint32_t)num_rx; sv.num_tx = (uint32_t)num_tx; sv.nr = (uint32_t)nr; sv.nt = (uint32_t)nt;
    sv.num_times = (uint32_t)num_times; sv.num_freqs = (uint32_t)num_freqs; sv.want = want;
    py::array_t<uint8_t> buf(fits ? (size_t)hrt_svd_out_bytes(&sv) : (size_t)1);
    uint8_t *dst = buf.mutable_data();
    const pattern_scope pattern_guard(patterns, num_rx, num_tx);
    run_pathsum("compute_channel_svd", mesh_filepath, [&](Scene *scene) {
        return hrt_compute_channel_svd(scene, e.rxp, e.txp, e.rxv, e.txv, carrier_frequency, num_rx, num_tx, num_paths,
                                       num_bounces, &spec, a.rxe, a.nr, a.txe, a.nt, fa, want, dst, nullptr);
    });
    size_t off = 0;
    auto view = [&](auto zero, std::vector<size_t> shape) {
        using T = decltype(zero);
        std::vector<py::ssize_t> strides(shape.size());
        py::ssize_t st = sizeof(T);
        size_t count = 1;
        for (size_t k = shape.size(); k-- > 0;) {
            strides[k] = st;
            st *= (py::ssize_t)shape[k];
            count *= shape[k];
        }
        py::array_t<T> v(shape, strides, reinterpret_cast<T *>(dst + off), buf);
        off += count * sizeof(T);
        return v;
    };
    const size_t R = num_rx, X = num_tx, T_ = num_times, K_ = num_freqs;
    py::dict d;
    d["sigma"] = view(0.0f, {R, X, n, 2, T_, K_});
    if (vectors) {
        d["u"] = view(std::complex<float>(), {R, X, nr, n, 2, T_, K_});
        d["v"] = view(std::complex<float>(), {R, X, nt, n, 2, T_, K_});
    } else {
        d["u"] = py::none();
        d["v"] = py::none();
    }
    d["sweeps"] = view((uint32_t)0, {R, X, 2, T_, K_});
    d["buffer"] = buf;
    return d;
}

// compute_channel_equalizer: the per-point linear MIMO equalizer (kind "zf" or "lmmse") of compute_array_channel's H and
// its post-equalisation SINR, formed on the device (extension; see hrt_compute_channel_equalizer in hermespy_rt.h): a
// dict of views of one buffer -- W complex64 (num_rx, num_tx, Nt, Nr, 2, num_times, num_freqs), None with
// weights=False; sinr float32 (num_rx, num_tx, Nt, 2, num_times, num_freqs); status uint32 (num_rx, num_tx, 2,
// num_times, num_freqs) -- and the buffer itself (uint8).  The equalizer is formed once, of the H of all batches.
py::dict compute_channel_equalizer_py(
    const std::string &mesh_filepath, farr rx_positions, farr tx_positions, farr rx_velocities, farr tx_velocities,
    float carrier_frequency, unsigned long num_rx, unsigned long num_tx, unsigned long num_paths,
    unsigned long num_bounces, double f0, double df, unsigned long num_freqs, farr rx_elements, farr tx_elements,
    float noise, const std::string &kind, double t0, double dt, unsigned long num_times, bool los, bool scatter,
    py::object array_frequency, bool weights, py::object patterns)
{
    const endpoints e(rx_positions, tx_positions, rx_velocities, tx_velocities, num_rx, num_tx, num_paths, num_bounces);
    if (num_freqs > 0xffffffffUL || num_times > 0xffffffffUL || num_rx > 0xffffffffUL || num_tx > 0xffffffffUL)
        throw std::invalid_argument("num_rx, num_tx, num_freqs and num_times must fit 32 bits");
    if (kind != "zf" && kind != "lmmse") throw std::invalid_argument("kind must be 'zf' or 'lmmse'");
    const array_elements a(rx_elements, tx_elements);
    const double fa = array_frequency.is_none() ? (double)carrier_frequency * 1e9 : array_frequency.cast<double>();
    check_scene_file(mesh_filepath);
    hrt_channel_spec spec{};
    spec.f0_hz = f0; spec.df_hz = df; spec.num_freqs = (uint32_t)num_freqs;
    spec.t0_s = t0; spec.dt_s = dt; spec.num_times = (uint32_t)num_times;
    spec.parts = parts_word(los, scatter);
    const uint32_t k = kind == "zf" ? HRT_EQ_ZF : HRT_EQ_LMMSE, flags = weights ? HRT_EQ_W : 0u;
    // (the library validates everything before it traces anything: a refused call raises ValueError; an output beyond
    // its limits is not allocated)
    const size_t nr = a.nr, nt = a.nt;
    const size_t pts = (size_t)num_rx * num_tx * 2u * num_times * num_freqs;
    const bool fits = a.fits((unsigned long long)num_times * num_freqs) && nt <= 16u && nr <= 64u && pts < (1ull << 31);
    hrt_equalizer_spec eq{};
    eq.num_rx = (uint32_t)num_rx; eq.num_tx = (uint32_t)num_tx; eq.nr = (uint32_t)nr; eq.nt = (uint32_t)nt;
    eq.num_times = (uint32_t)num_times; eq.num_freqs = (uint32_t)num_freqs; eq.kind = k; eq.flags = flags;
    eq.noise = noise;
    py::array_t<uint8_t> buf(fits ? (size_t)hrt_equalizer_out_bytes(&eq) : (size_t)1);
    uint8_t *dst = buf.mutable_data();
    const pattern_scope pattern_guard(patterns, num_rx, num_tx);
    run_pathsum("compute_channel_equalizer", mesh_filepath, [&](Scene *scene) {
        return hrt_compute_channel_equalizer(scene, e.rxp, e.txp, e.rxv, e.txv, carrier_frequency, num_rx, num_tx,
                                             num_paths, num_bounces, &spec, a.rxe, a.nr, a.txe, a.nt, fa, k, flags,
                                             noise, dst, nullptr);
    });
    size_t off = 0;
    auto view = [&](auto zero, std::vector<size_t> shape) {
        using T = decltype(zero);
        std::vector<py::ssize_t> strides(shape.size());
        py::ssize_t st = sizeof(T);
        size_t count = 1;
        for (size_t i = shape.size(); i-- > 0;) {
            strides[i] = st;
            st *= (py::ssize_t)shape[i];
            count *= shape[i];
        }
        py::array_t<T> v(shape, strides, reinterpret_cast<T *>(dst + off), buf);
        off += count * sizeof(T);
        return v;
    };
    const size_t R = num_rx, X = num_tx, T_ = num_times, K_ = num_freqs;
    py::dict d;
    if (weights) d["W"] = view(std::complex<float>(), {R, X, nt, nr, 2, T_, K_});
    else d["W"] = py::none();
    d["sinr"] = view(0.0f, {R, X, nt, 2, T_, K_});
    d["status"] = view((uint32_t)0, {R, X, 2, T_, K_});
    d["buffer"] = buf;
    return d;
}

// compute_channel_precoder: the per-point linear MIMO precoder (kind "mrt", "zf" or "rzf"; normalize "total" or "stream")
// of compute_array_channel's H and the downlink SINR of every stream behind it, formed on the device (extension; see
// hrt_compute_channel_precoder in hermespy_rt.h): a dict of views of one buffer -- P complex64 (num_rx, num_tx, Nt, Nr,
// 2, num_times, num_freqs), None with weights=False; sinr float32 (num_rx, num_tx, Nr, 2, num_times, num_freqs); status
// uint32 (num_rx, num_tx, 2, num_times, num_freqs) -- and the buffer itself (uint8).  regularization None: Nr noise /
// power under "rzf".  The precoder is formed once, of the H of all batches.
py::dict compute_channel_precoder_py(
    const std::string &mesh_filepath, farr rx_positions, farr tx_positions, farr rx_velocities, farr tx_velocities,
    float carrier_frequency, unsigned long num_rx, unsigned long num_tx, unsigned long num_paths,
    unsigned long num_bounces, double f0, double df, unsigned long num_freqs, farr rx_elements, farr tx_elements,
    float noise, const std::string &kind, float power, py::object regularization, const std::string &normalize,
    double t0, double dt, unsigned long num_times, bool los, bool scatter, py::object array_frequency, bool weights,
    py::object patterns)
{
    const endpoints e(rx_positions, tx_positions, rx_velocities, tx_velocities, num_rx, num_tx, num_paths, num_bounces);
    if (num_freqs > 0xffffffffUL || num_times > 0xffffffffUL || num_rx > 0xffffffffUL || num_tx > 0xffffffffUL)
        throw std::invalid_argument("num_rx, num_tx, num_freqs and num_times must fit 32 bits");
    if (kind != "mrt" && kind != "zf" && kind != "rzf") throw std::invalid_argument("kind must be 'mrt', 'zf' or 'rzf'");
    if (normalize != "total" && normalize != "stream")
        throw std::invalid_argument("normalize must be 'total' or 'stream'");
    const array_elements a(rx_elements, tx_elements);
    const double fa = array_frequency.is_none() ? (double)carrier_frequency * 1e9 : array_frequency.cast<double>();
    check_scene_file(mesh_filepath);
    hrt_channel_spec spec{};
    spec.f0_hz = f0; spec.df_hz = df; spec.num_freqs = (uint32_t)num_freqs;
    spec.t0_s = t0; spec.dt_s = dt; spec.num_times = (uint32_t)num_times;
    spec.parts = parts_word(los, scatter);
    const uint32_t k = kind == "mrt" ? HRT_PC_MRT : kind == "zf" ? HRT_PC_ZF : HRT_PC_RZF;
    const uint32_t norm = normalize == "total" ? HRT_PC_TOTAL : HRT_PC_STREAM, flags = weights ? HRT_PC_P : 0u;
    const size_t nr = a.nr, nt = a.nt;
    float alpha = 0.f;
    if (!regularization.is_none()) alpha = regularization.cast<float>();
    else if (k == HRT_PC_RZF && power > 0.f) alpha = (float)((double)nr * (double)noise / (double)power);
    // (the library validates everything before it traces anything: a refused call raises ValueError; an output beyond
    // its limits is not allocated)
    const size_t pts = (size_t)num_rx * num_tx * 2u * num_times * num_freqs;
    const bool fits = a.fits((unsigned long long)num_times * num_freqs) && nr <= 16u && nt <= 64u && pts < (1ull << 31);
    hrt_precoder_spec pc{};
    pc.num_rx = (uint32_t)num_rx; pc.num_tx = (uint32_t)num_tx; pc.nr = (uint32_t)nr; pc.nt = (uint32_t)nt;
    pc.num_times = (uint32_t)num_times; pc.num_freqs = (uint32_t)num_freqs; pc.kind = k; pc.norm = norm;
    pc.flags = flags; pc.noise = noise; pc.power = power; pc.regularization = alpha;
    py::array_t<uint8_t> buf(fits ? (size_t)hrt_precoder_out_bytes(&pc) : (size_t)1);
    uint8_t *dst = buf.mutable_data();
    const pattern_scope pattern_guard(patterns, num_rx, num_tx);
    run_pathsum("compute_channel_precoder", mesh_filepath, [&](Scene *scene) {
        return hrt_compute_channel_precoder(scene, e.rxp, e.txp, e.rxv, e.txv, carrier_frequency, num_rx, num_tx,
                                            num_paths, num_bounces, &spec, a.rxe, a.nr, a.txe, a.nt, fa, k, norm, flags,
                                            noise, power, alpha, dst, nullptr);
    });
    size_t off = 0;
    auto view = [&](auto zero, std::vector<size_t> shape) {
        using T = decltype(zero);
        std::vector<py::ssize_t> strides(shape.size());
        py::ssize_t st = sizeof(T);
        size_t count = 1;
        for (size_t i = shape.size(); i-- > 0;) {
            strides[i] = st;
            st *= (py::ssize_t)shape[i];
            count *= shape[i];
        }
        py::array_t<T> v(shape, strides, reinterpret_cast<T *>(dst + off), buf);
        off += count * sizeof(T);
        return v;
    };
    const size_t R = num_rx, X = num_tx, T_ = num_times, K_ = num_freqs;
    py::dict d;
    if (weights) d["P"] = view(std::complex<float>(), {R, X, nt, nr, 2, T_, K_});
    else d["P"] = py::none();
    d["sinr"] = view(0.0f, {R, X, nr, 2, T_, K_});
    d["status"] = view((uint32_t)0, {R, X, 2, T_, K_});
    d["buffer"] = buf;
    return d;
}

// compute_codebook_select: per-subband precoder codebook selection (metric "power" or "capacity") on
// compute_array_channel's H, formed on the device (extension; see hrt_compute_codebook_select in hermespy_rt.h): a dict of
// views of one buffer -- index uint32, metric float32 and status uint32 (num_rx, num_tx, 2, num_times, B); table float32
// (num_rx, num_tx, C, 2, num_times, B), None without table=True; effective complex64 (num_rx, num_tx, Nr, L, 2, num_times,
// num_freqs), None without effective=True -- and the buffer itself (uint8).  codebook: complex64 (C, Nt, L) or (C, Nt);
// subband None: wideband.  The selection runs once, on the H of all batches.
py::dict compute_codebook_select_py(
    const std::string &mesh_filepath, farr rx_positions, farr tx_positions, farr rx_velocities, farr tx_velocities,
    float carrier_frequency, unsigned long num_rx, unsigned long num_tx, unsigned long num_paths,
    unsigned long num_bounces, double f0, double df, unsigned long num_freqs, farr rx_elements, farr tx_elements,
    py::array codebook, const std::string &metric, py::object noise, py::object subband, double t0, double dt,
    unsigned long num_times, bool los, bool scatter, py::object array_frequency, bool table, bool effective,
    py::object patterns)
{
    const endpoints e(rx_positions, tx_positions, rx_velocities, tx_velocities, num_rx, num_tx, num_paths, num_bounces);
    if (num_freqs > 0xffffffffUL || num_times > 0xffffffffUL || num_rx > 0xffffffffUL || num_tx > 0xffffffffUL)
        throw std::invalid_argument("num_rx, num_tx, num_freqs and num_times must fit 32 bits");
    if (metric != "power" && metric != "capacity") throw std::invalid_argument("metric must be 'power' or 'capacity'");
    const array_elements a(rx_elements, tx_elements);
    const size_t nr = a.nr, nt = a.nt;
    if (codebook.ndim() != 2 && codebook.ndim() != 3)
        throw std::invalid_argument("codebook must have shape (C, Nt, L) or (C, Nt)");
    const auto cb = py::array_t<std::complex<float>, py::array::c_style | py::array::forcecast>::ensure(codebook);
    if (!cb) throw std::invalid_argument("codebook must be a complex array");
    const size_t C_ = (size_t)cb.shape(0), L_ = cb.ndim() == 3 ? (size_t)cb.shape(2) : 1u;
    if ((size_t)cb.shape(1) != nt) throw std::invalid_argument("codebook must have shape (C, Nt, L) with Nt tx_elements");
    if (C_ > 0xffffffffUL || L_ > 0xffffffffUL) throw std::invalid_argument("codebook too large");
    const double fa = array_frequency.is_none() ? (double)carrier_frequency * 1e9 : array_frequency.cast<double>();
    check_scene_file(mesh_filepath);
    hrt_channel_spec spec{};
    spec.f0_hz = f0; spec.df_hz = df; spec.num_freqs = (uint32_t)num_freqs;
    spec.t0_s = t0; spec.dt_s = dt; spec.num_times = (uint32_t)num_times;
    spec.parts = parts_word(los, scatter);
    const uint32_t mt = metric == "power" ? HRT_CS_POWER : HRT_CS_CAPACITY;
    const uint32_t flags = (table ? HRT_CS_TABLE : 0u) | (effective ? HRT_CS_EFFECTIVE : 0u);
    const float n0 = noise.is_none() ? (mt == HRT_CS_POWER ? 1.f : 0.f) : noise.cast<float>();
    unsigned long S = num_freqs;
    if (!subband.is_none()) {
        const long long sv = subband.cast<long long>();
        if (sv < 0 || sv > 0xffffffffLL) throw std::invalid_argument("subband must fit 32 bits");
        S = (unsigned long)sv;
    }
    hrt_codebook_spec cs{};
    cs.num_rx = (uint32_t)num_rx; cs.num_tx = (uint32_t)num_tx; cs.nr = (uint32_t)nr; cs.nt = (uint32_t)nt;
    cs.num_times = (uint32_t)num_times; cs.num_freqs = (uint32_t)num_freqs; cs.layers = (uint32_t)L_;
    cs.entries = (uint32_t)C_; cs.subband = (uint32_t)S; cs.metric = mt; cs.flags = flags; cs.noise = n0;
    // (the library validates everything before it traces anything: a refused call raises ValueError; an output beyond
    // its limits is not allocated)
    const size_t pts = (size_t)num_rx * num_tx * 2u * num_times * num_freqs;
    const size_t B_ = S ? (num_freqs + S - 1u) / S : 0u;
    const bool fits = a.fits((unsigned long long)num_times * num_freqs) && nr <= 16u && nt <= 64u && L_ >= 1u && L_ <= 4u
                      && C_ >= 1u && C_ <= 4096u && S >= 1u && S <= num_freqs && pts < (1ull << 31)
                      && (unsigned long long)num_rx * num_tx * 2u * num_times * B_ * C_ < (1ull << 31);
    py::array_t<uint8_t> buf(fits ? (size_t)hrt_codebook_out_bytes(&cs) : (size_t)1);
    uint8_t *dst = buf.mutable_data();
    const pattern_scope pattern_guard(patterns, num_rx, num_tx);
    run_pathsum("compute_codebook_select", mesh_filepath, [&](Scene *scene) {
        return hrt_compute_codebook_select(scene, e.rxp, e.txp, e.rxv, e.txv, carrier_frequency, num_rx, num_tx,
                                           num_paths, num_bounces, &spec, a.rxe, a.nr, a.txe, a.nt, fa,
                                           reinterpret_cast<const float *>(cb.data()), cs.layers, cs.entries, cs.subband,
                                           mt, flags, n0, dst, nullptr);
    });
    size_t off = 0;
    auto view = [&](auto zero, std::vector<size_t> shape) {
        using T = decltype(zero);
        std::vector<py::ssize_t> strides(shape.size());
        py::ssize_t st = sizeof(T);
        size_t count = 1;
        for (size_t i = shape.size(); i-- > 0;) {
            strides[i] = st;
            st *= (py::ssize_t)shape[i];
            count *= shape[i];
        }
        py::array_t<T> v(shape, strides, reinterpret_cast<T *>(dst + off), buf);
        off += count * sizeof(T);
        return v;
    };
    const size_t R = num_rx, X = num_tx, T_ = num_times, K_ = num_freqs;
    py::dict d;
    d["index"] = view((uint32_t)0, {R, X, 2, T_, B_});
    d["metric"] = view(0.0f, {R, X, 2, T_, B_});
    d["status"] = view((uint32_t)0, {R, X, 2, T_, B_});
    if (table) d["table"] = view(0.0f, {R, X, C_, 2, T_, B_});
    else d["table"] = py::none();
    if (effective) d["effective"] = view(std::complex<float>(), {R, X, nr, L_, 2, T_, K_});
    else d["effective"] = py::none();
    d["buffer"] = buf;
    return d;
}

// compute_channel_detect: per-point maximum-likelihood detection with max-log bit LLRs on compute_array_channel's H,
// formed on the device (extension; see hrt_compute_channel_detect in hermespy_rt.h): a dict of views of one buffer --
// index uint32, metric float32 and status uint32 (num_rx, num_tx, 2, num_times, num_freqs); llr float32 (num_rx,
// num_tx, Nt, B, 2, num_times, num_freqs), None without llr=True -- and the buffer itself (uint8).  Y: complex64
// (num_rx, num_tx, Nr, 2, num_times, num_freqs); constellation: complex64 (2^B,).  Detection runs once, on the H of
// all batches.
py::dict compute_channel_detect_py(
    const std::string &mesh_filepath, farr rx_positions, farr tx_positions, farr rx_velocities, farr tx_velocities,
    float carrier_frequency, unsigned long num_rx, unsigned long num_tx, unsigned long num_paths,
    unsigned long num_bounces, double f0, double df, unsigned long num_freqs, farr rx_elements, farr tx_elements,
    py::array Y, py::array constellation, float noise, double t0, double dt, unsigned long num_times, bool los,
    bool scatter, py::object array_frequency, bool llr, py::object patterns)
{
    const endpoints e(rx_positions, tx_positions, rx_velocities, tx_velocities, num_rx, num_tx, num_paths, num_bounces);
    if (num_freqs > 0xffffffffUL || num_times > 0xffffffffUL || num_rx > 0xffffffffUL || num_tx > 0xffffffffUL)
        throw std::invalid_argument("num_rx, num_tx, num_freqs and num_times must fit 32 bits");
    const array_elements a(rx_elements, tx_elements);
    const size_t nr = a.nr, nt = a.nt;
    using cf = py::array_t<std::complex<float>, py::array::c_style | py::array::forcecast>;
    const auto sy = cf::ensure(constellation);
    if (!sy || sy.ndim() != 1) throw std::invalid_argument("constellation must be a complex array of shape (M,)");
    const size_t M_ = (size_t)sy.shape(0);
    uint32_t bits = 0;
    while (bits < 31u && ((size_t)1 << bits) < M_) ++bits;
    if (M_ < 2u || ((size_t)1 << bits) != M_) throw std::invalid_argument("constellation must hold 2^B symbols");
    const auto yy = cf::ensure(Y);
    if (!yy || yy.ndim() != 6 || (size_t)yy.shape(0) != num_rx || (size_t)yy.shape(1) != num_tx
        || (size_t)yy.shape(2) != nr || yy.shape(3) != 2 || (size_t)yy.shape(4) != num_times
        || (size_t)yy.shape(5) != num_freqs)
        throw std::invalid_argument("Y must be a complex array of shape (num_rx, num_tx, Nr, 2, num_times, num_freqs)");
    const double fa = array_frequency.is_none() ? (double)carrier_frequency * 1e9 : array_frequency.cast<double>();
    check_scene_file(mesh_filepath);
    hrt_channel_spec spec{};
    spec.f0_hz = f0; spec.df_hz = df; spec.num_freqs = (uint32_t)num_freqs;
    spec.t0_s = t0; spec.dt_s = dt; spec.num_times = (uint32_t)num_times;
    spec.parts = parts_word(los, scatter);
    const uint32_t flags = llr ? HRT_DT_LLR : 0u;
    hrt_detect_spec ds{};
    ds.num_rx = (uint32_t)num_rx; ds.num_tx = (uint32_t)num_tx; ds.nr = (uint32_t)nr; ds.nt = (uint32_t)nt;
    ds.num_times = (uint32_t)num_times; ds.num_freqs = (uint32_t)num_freqs; ds.bits = bits; ds.flags = flags;
    ds.noise = noise;
    // (the library validates everything before it traces anything: a refused call raises ValueError; an output beyond
    // its limits is not allocated)
    const size_t pts = (size_t)num_rx * num_tx * 2u * num_times * num_freqs;
    const bool fits = a.fits((unsigned long long)num_times * num_freqs) && nr <= 64u && bits >= 1u && bits <= 8u
                      && nt * bits <= 12u && pts < (1ull << 31);
    py::array_t<uint8_t> buf(fits ? (size_t)hrt_detect_out_bytes(&ds) : (size_t)1);
    uint8_t *dst = buf.mutable_data();
    const pattern_scope pattern_guard(patterns, num_rx, num_tx);
    run_pathsum("compute_channel_detect", mesh_filepath, [&](Scene *scene) {
        return hrt_compute_channel_detect(scene, e.rxp, e.txp, e.rxv, e.txv, carrier_frequency, num_rx, num_tx,
                                          num_paths, num_bounces, &spec, a.rxe, a.nr, a.txe, a.nt, fa,
                                          reinterpret_cast<const float *>(yy.data()),
                                          reinterpret_cast<const float *>(sy.data()), bits, flags, noise, dst, nullptr);
    });
    size_t off = 0;
    auto view = [&](auto zero, std::vector<size_t> shape) {
        using T = decltype(zero);
        std::vector<py::ssize_t> strides(shape.size());
        py::ssize_t st = sizeof(T);
        size_t count = 1;
        for (size_t i = shape.size(); i-- > 0;) {
            strides[i] = st;
            st *= (py::ssize_t)shape[i];
            count *= shape[i];
        }
        py::array_t<T> v(shape, strides, reinterpret_cast<T *>(dst + off), buf);
        off += count * sizeof(T);
        return v;
    };
    const size_t R = num_rx, X = num_tx, T_ = num_times, K_ = num_freqs;
    py::dict d;
    d["index"] = view((uint32_t)0, {R, X, 2, T_, K_});
    d["metric"] = view(0.0f, {R, X, 2, T_, K_});
    d["status"] = view((uint32_t)0, {R, X, 2, T_, K_});
    if (llr) d["llr"] = view(0.0f, {R, X, nt, (size_t)bits, 2, T_, K_});
    else d["llr"] = py::none();
    d["buffer"] = buf;
    return d;
}

// compute_channel_kbest: per-point K-best tree-search detection with list max-log bit LLRs on compute_array_channel's
// H, formed on the device (extension; see hrt_compute_channel_kbest in hermespy_rt.h): the dict of
// compute_channel_detect -- index, metric, status, llr (None without llr=True), buffer.  k: the list size (1, 2, 4, ..
// 64); clip: the LLR clip; sorted: sorted QR.  Detection runs once, on the H of all batches.
py::dict compute_channel_kbest_py(
    const std::string &mesh_filepath, farr rx_positions, farr tx_positions, farr rx_velocities, farr tx_velocities,
    float carrier_frequency, unsigned long num_rx, unsigned long num_tx, unsigned long num_paths,
    unsigned long num_bounces, double f0, double df, unsigned long num_freqs, farr rx_elements, farr tx_elements,
    py::array Y, py::array constellation, float noise, unsigned long k, float clip, double t0, double dt,
    unsigned long num_times, bool los, bool scatter, py::object array_frequency, bool sorted, bool llr,
    py::object patterns)
{
    const endpoints e(rx_positions, tx_positions, rx_velocities, tx_velocities, num_rx, num_tx, num_paths, num_bounces);
    if (num_freqs > 0xffffffffUL || num_times > 0xffffffffUL || num_rx > 0xffffffffUL || num_tx > 0xffffffffUL
        || k > 0xffffffffUL)
        throw std::invalid_argument("num_rx, num_tx, num_freqs, num_times and k must fit 32 bits");
    const array_elements a(rx_elements, tx_elements);
    const size_t nr = a.nr, nt = a.nt;
    using cf = py::array_t<std::complex<float>, py::array::c_style | py::array::forcecast>;
    const auto sy = cf::ensure(constellation);
    if (!sy || sy.ndim() != 1) throw std::invalid_argument("constellation must be a complex array of shape (M,)");
    const size_t M_ = (size_t)sy.shape(0);
    uint32_t bits = 0;
    while (bits < 31u && ((size_t)1 << bits) < M_) ++bits;
    if (M_ < 2u || ((size_t)1 << bits) != M_) throw std::invalid_argument("constellation must hold 2^B symbols");
    const auto yy = cf::ensure(Y);
    if (!yy || yy.ndim() != 6 || (size_t)yy.shape(0) != num_rx || (size_t)yy.shape(1) != num_tx
        || (size_t)yy.shape(2) != nr || yy.shape(3) != 2 || (size_t)yy.shape(4) != num_times
        || (size_t)yy.shape(5) != num_freqs)
        throw std::invalid_argument("Y must be a complex array of shape (num_rx, num_tx, Nr, 2, num_times, num_freqs)");
    const double fa = array_frequency.is_none() ? (double)carrier_frequency * 1e9 : array_frequency.cast<double>();
    check_scene_file(mesh_filepath);
    hrt_channel_spec spec{};
    spec.f0_hz = f0; spec.df_hz = df; spec.num_freqs = (uint32_t)num_freqs;
    spec.t0_s = t0; spec.dt_s = dt; spec.num_times = (uint32_t)num_times;
    spec.parts = parts_word(los, scatter);
    const uint32_t flags = (llr ? HRT_KB_LLR : 0u) | (sorted ? HRT_KB_SORTED : 0u);
    hrt_kbest_spec ks{};
    ks.num_rx = (uint32_t)num_rx; ks.num_tx = (uint32_t)num_tx; ks.nr = (uint32_t)nr; ks.nt = (uint32_t)nt;
    ks.num_times = (uint32_t)num_times; ks.num_freqs = (uint32_t)num_freqs; ks.bits = bits; ks.flags = flags;
    ks.k = (uint32_t)k; ks.noise = noise; ks.clip = clip;
    // (the library validates everything before it traces anything: a refused call raises ValueError; an output beyond
    // its limits is not allocated)
    const size_t pts = (size_t)num_rx * num_tx * 2u * num_times * num_freqs;
    const bool fits = a.fits((unsigned long long)num_times * num_freqs) && nr <= 64u && nt <= 16u && bits >= 1u
                      && bits <= 8u && nt * bits <= 32u && pts < (1ull << 31);
    py::array_t<uint8_t> buf(fits ? (size_t)hrt_kbest_out_bytes(&ks) : (size_t)1);
    uint8_t *dst = buf.mutable_data();
    const pattern_scope pattern_guard(patterns, num_rx, num_tx);
    run_pathsum("compute_channel_kbest", mesh_filepath, [&](Scene *scene) {
        return hrt_compute_channel_kbest(scene, e.rxp, e.txp, e.rxv, e.txv, carrier_frequency, num_rx, num_tx,
                                         num_paths, num_bounces, &spec, a.rxe, a.nr, a.txe, a.nt, fa,
                                         reinterpret_cast<const float *>(yy.data()),
                                         reinterpret_cast<const float *>(sy.data()), bits, flags, (uint32_t)k, noise,
                                         clip, dst, nullptr);
    });
    size_t off = 0;
    auto view = [&](auto zero, std::vector<size_t> shape) {
        using T = decltype(zero);
        std::vector<py::ssize_t> strides(shape.size());
        py::ssize_t st = sizeof(T);
        size_t count = 1;
        for (size_t i = shape.size(); i-- > 0;) {
            strides[i] = st;
            st *= (py::ssize_t)shape[i];
            count *= shape[i];
        }
        py::array_t<T> v(shape, strides, reinterpret_cast<T *>(dst + off), buf);
        off += count * sizeof(T);
        return v;
    };
    const size_t R = num_rx, X = num_tx, T_ = num_times, K_ = num_freqs;
    py::dict d;
    d["index"] = view((uint32_t)0, {R, X, 2, T_, K_});
    d["metric"] = view(0.0f, {R, X, 2, T_, K_});
    d["status"] = view((uint32_t)0, {R, X, 2, T_, K_});
    if (llr) d["llr"] = view(0.0f, {R, X, nt, (size_t)bits, 2, T_, K_});
    else d["llr"] = py::none();
    d["buffer"] = buf;
    return d;
}

// a codebook argument of compute_beam_channel: complex64 (beams, n_elements), C-contiguous (copied if it is not)
using carr = py::array_t<std::complex<float>, py::array::c_style>;
carr as_weights(const py::array &w, size_t n_elements, const char *name)
{
    if (!py::isinstance<py::array_t<std::complex<float>>>(w) || w.ndim() != 2 || (size_t)w.shape(1) != n_elements)
        throw std::invalid_argument(std::string(name) + " must be a complex64 array of shape (beams, " +
                                    std::to_string(n_elements) + ")");
    return carr::ensure(w);
}

// compute_beam_channel: the beamformed (codebook) channel of the traced paths, formed on the device (extension; see
// hrt_compute_beam_channel in hermespy_rt.h): complex64 (num_rx, num_tx, Br, Bt, 2, num_times, num_freqs) =
// sum_ij conj(rx_weights[a, i]) H[..., i, j, ...] tx_weights[b, j] of compute_array_channel's H, which is never formed.
py::array_t<std::complex<float>> compute_beam_channel_py(
    const std::string &mesh_filepath, farr rx_positions, farr tx_positions, farr rx_velocities, farr tx_velocities,
    float carrier_frequency, unsigned long num_rx, unsigned long num_tx, unsigned long num_paths,
    unsigned long num_bounces, double f0, double df, unsigned long num_freqs, farr rx_elements, farr tx_elements,
    py::array rx_weights, py::array tx_weights, double t0, double dt, unsigned long num_times, bool los, bool scatter,
    py::object array_frequency,
    py::object patterns)
{
    const endpoints e(rx_positions, tx_positions, rx_velocities, tx_velocities, num_rx, num_tx, num_paths, num_bounces);
    if (num_freqs > 0xffffffffUL || num_times > 0xffffffffUL)
        throw std::invalid_argument("num_freqs and num_times must fit 32 bits");
    const array_elements a(rx_elements, tx_elements);
    const carr wr = as_weights(rx_weights, a.nr, "rx_weights"), wt = as_weights(tx_weights, a.nt, "tx_weights");
    const size_t br = (size_t)wr.shape(0), bt = (size_t)wt.shape(0);
    const double fa = array_frequency.is_none() ? (double)carrier_frequency * 1e9 : array_frequency.cast<double>();
    check_scene_file(mesh_filepath);
    hrt_channel_spec spec{};
    spec.f0_hz = f0; spec.df_hz = df; spec.num_freqs = (uint32_t)num_freqs;
    spec.t0_s = t0; spec.dt_s = dt; spec.num_times = (uint32_t)num_times;
    spec.parts = parts_word(los, scatter);
    // (the library validates everything before it traces anything: a refused call raises ValueError.  An output
    // beyond the 2^24 points of the limit would be refused, so only one within it is allocated.)
    const unsigned long long pts = (unsigned long long)br * bt * num_times * num_freqs;
    const bool fits = pts > 0 && pts <= (1ull << 24) && br <= 256 && bt <= 256;
    py::array_t<std::complex<float>> out(fits ? std::vector<size_t>{(size_t)num_rx, (size_t)num_tx, br, bt, (size_t)2,
                                                                    (size_t)num_times, (size_t)num_freqs}
                                              : std::vector<size_t>{1});
    float *dst = reinterpret_cast<float *>(out.mutable_data());
    const float *pwr = reinterpret_cast<const float *>(wr.data()), *pwt = reinterpret_cast<const float *>(wt.data());
    const pattern_scope pattern_guard(patterns, num_rx, num_tx);
    run_pathsum("compute_beam_channel", mesh_filepath, [&](Scene *scene) {
        return hrt_compute_beam_channel(scene, e.rxp, e.txp, e.rxv, e.txv, carrier_frequency, num_rx, num_tx, num_paths,
                                        num_bounces, &spec, a.rxe, a.nr, a.txe, a.nt, fa, pwr, br, pwt, bt, dst,
                                        nullptr);
    });
    return out;
}

// compute_taps: the sampled channel impulse response of the traced paths, formed on the device (extension; see
// hrt_compute_taps in hermespy_rt.h): complex64 (num_rx, num_tx, 2, num_times, num_taps),
// h = sum_p a_p exp(j 2 pi (nu_p t_m - f_c tau_p)) sinc(l_i - f_s tau_p), l_i = l_min + i; center_frequency f_c (Hz)
// defaults to the carrier.
py::array_t<std::complex<float>> compute_taps_py(
    const std::string &mesh_filepath, farr rx_positions, farr tx_positions, farr rx_velocities, farr tx_velocities,
    float carrier_frequency, unsigned long num_rx, unsigned long num_tx, unsigned long num_paths,
    unsigned long num_bounces, double sampling_rate, unsigned long num_taps, long l_min, py::object center_frequency,
    double t0, double dt, unsigned long num_times, bool los, bool scatter,
    py::object patterns)
{
    const endpoints e(rx_positions, tx_positions, rx_velocities, tx_velocities, num_rx, num_tx, num_paths, num_bounces);
    if (num_taps > 0xffffffffUL || num_times > 0xffffffffUL)
        throw std::invalid_argument("num_taps and num_times must fit 32 bits");
    if (l_min < -(1L << 30) || l_min > (1L << 30))
        throw py::value_error("hermespy_rt.compute_taps: tap indices l_min outside +-2^24");
    const double fc = center_frequency.is_none() ? (double)carrier_frequency * 1e9 : center_frequency.cast<double>();
    check_scene_file(mesh_filepath);
    hrt_taps_spec spec{};
    spec.fs_hz = sampling_rate; spec.fc_hz = fc; spec.t0_s = t0; spec.dt_s = dt;
    spec.l_min = (int32_t)l_min; spec.num_taps = (uint32_t)num_taps; spec.num_times = (uint32_t)num_times;
    spec.parts = parts_word(los, scatter);
    // (the library validates the spec before it traces anything: a refused one raises ValueError; an output too
    // large for its limits is not allocated)
    const bool fits = num_taps && num_times && (uint64_t)num_taps * num_times <= (1ull << 20);
    py::array_t<std::complex<float>> out(fits ? std::vector<size_t>{(size_t)num_rx, (size_t)num_tx, (size_t)2,
                                                                     (size_t)num_times, (size_t)num_taps}
                                              : std::vector<size_t>{(size_t)1});
    float *dst = reinterpret_cast<float *>(out.mutable_data());
    const pattern_scope pattern_guard(patterns, num_rx, num_tx);
    run_pathsum("compute_taps", mesh_filepath, [&](Scene *scene) {
        return hrt_compute_taps(scene, e.rxp, e.txp, e.rxv, e.txv, carrier_frequency, num_rx, num_tx, num_paths, num_bounces,
                                &spec, dst, nullptr);
    });
    return out;
}

// compute_array_taps: the antenna-array sampled impulse response of the traced paths, formed on the device
// (extension; see hrt_compute_array_taps in hermespy_rt.h): complex64 (num_rx, num_tx, Nr, Nt, 2, num_times,
// num_taps).  Element offsets are (Nr, 3) / (Nt, 3) metres from the traced RX / TX positions; center_frequency f_c
// and array_frequency f_a (Hz) default to the carrier.
py::array_t<std::complex<float>> compute_array_taps_py(
    const std::string &mesh_filepath, farr rx_positions, farr tx_positions, farr rx_velocities, farr tx_velocities,
    float carrier_frequency, unsigned long num_rx, unsigned long num_tx, unsigned long num_paths,
    unsigned long num_bounces, double sampling_rate, unsigned long num_taps, farr rx_elements, farr tx_elements,
    long l_min, py::object center_frequency, double t0, double dt, unsigned long num_times, bool los, bool scatter,
    py::object array_frequency,
    py::object patterns)
{
    const endpoints e(rx_positions, tx_positions, rx_velocities, tx_velocities, num_rx, num_tx, num_paths, num_bounces);
    if (num_taps > 0xffffffffUL || num_times > 0xffffffffUL)
        throw std::invalid_argument("num_taps and num_times must fit 32 bits");
    if (l_min < -(1L << 30) || l_min > (1L << 30))
        throw py::value_error("hermespy_rt.compute_array_taps: tap indices l_min outside +-2^24");
    const array_elements a(rx_elements, tx_elements);
    const double fc = center_frequency.is_none() ? (double)carrier_frequency * 1e9 : center_frequency.cast<double>();
    const double fa = array_frequency.is_none() ? (double)carrier_frequency * 1e9 : array_frequency.cast<double>();
    check_scene_file(mesh_filepath);
    hrt_taps_spec spec{};
    spec.fs_hz = sampling_rate; spec.fc_hz = fc; spec.t0_s = t0; spec.dt_s = dt;
    spec.l_min = (int32_t)l_min; spec.num_taps = (uint32_t)num_taps; spec.num_times = (uint32_t)num_times;
    spec.parts = parts_word(los, scatter);
    // (the library validates everything before it traces anything: a refused call raises ValueError.  An output
    // beyond the limits would be refused, so only one within them is allocated.)
    const bool fits = a.fits((unsigned long long)num_times * num_taps) && (uint64_t)num_taps * num_times <= (1ull << 20);
    py::array_t<std::complex<float>> out(fits ? std::vector<size_t>{(size_t)num_rx, (size_t)num_tx, a.nr, a.nt, (size_t)2,
                                                                    (size_t)num_times, (size_t)num_taps}
                                              : std::vector<size_t>{1});
    float *dst = reinterpret_cast<float *>(out.mutable_data());
    const pattern_scope pattern_guard(patterns, num_rx, num_tx);
    run_pathsum("compute_array_taps", mesh_filepath, [&](Scene *scene) {
        return hrt_compute_array_taps(scene, e.rxp, e.txp, e.rxv, e.txv, carrier_frequency, num_rx, num_tx, num_paths,
                                      num_bounces, &spec, a.rxe, a.nr, a.txe, a.nt, fa, dst, nullptr);
    });
    return out;
}

// compute_received_signal: the samples the receivers see when the transmitters send `signal` through the traced
// channel (extension; see hrt_compute_received_signal in hermespy_rt.h): complex64 (num_rx, Nr, 2, num_out).  signal is
// complex (num_tx, Nt, N), or (num_tx, N) with Nt = 1.  The channel is block-wise time-variant: M = ceil(num_out /
// samples_per_block) blocks formed at their centres, t0 = t_start + (S - 1) / (2 f_s), dt = S / f_s;
// samples_per_block None is the time-invariant channel at t_start.  num_out defaults to N + num_taps - 1 + max(l_min, 0).
// The taps stay on the device; only the signal comes back.
py::array_t<std::complex<float>> compute_received_signal_py(
    const std::string &mesh_filepath, farr rx_positions, farr tx_positions, farr rx_velocities, farr tx_velocities,
    float carrier_frequency, unsigned long num_rx, unsigned long num_tx, unsigned long num_paths,
    unsigned long num_bounces, double sampling_rate, unsigned long num_taps, farr rx_elements, farr tx_elements,
    py::array_t<std::complex<float>, py::array::c_style | py::array::forcecast> signal, long l_min,
    py::object samples_per_block, double t_start, py::object center_frequency, py::object num_out, bool los,
    bool scatter, py::object array_frequency,
    py::object patterns)
{
    const endpoints e(rx_positions, tx_positions, rx_velocities, tx_velocities, num_rx, num_tx, num_paths, num_bounces);
    if (num_taps > 0xffffffffUL) throw std::invalid_argument("num_taps must fit 32 bits");
    if (l_min < -(1L << 30) || l_min > (1L << 30))
        throw py::value_error("hermespy_rt.compute_received_signal: tap indices l_min outside +-2^24");
    const array_elements a(rx_elements, tx_elements);
    if (signal.ndim() != 2 && signal.ndim() != 3)
        throw std::invalid_argument("signal must have shape (num_tx, Nt, N) or (num_tx, N)");
    const size_t n = (size_t)signal.shape(signal.ndim() - 1);
    const size_t ports = signal.ndim() == 3 ? (size_t)signal.shape(0) * (size_t)signal.shape(1) : (size_t)signal.shape(0);
    if (ports != (size_t)num_tx * a.nt || (signal.ndim() == 3 && (size_t)signal.shape(0) != num_tx))
        throw std::invalid_argument("signal must have num_tx x Nt TX ports");
    const uint64_t n_out = num_out.is_none() ? (uint64_t)n + num_taps - 1u + (uint64_t)(l_min > 0 ? l_min : 0)
                                             : num_out.cast<uint64_t>();
    uint64_t s = n_out ? n_out : 1u, m = 1;
    double t0 = t_start, dt = 0.0;
    if (!samples_per_block.is_none()) {
        s = samples_per_block.cast<uint64_t>();
        if (s > 0xffffffffULL) throw std::invalid_argument("samples_per_block must fit 32 bits");
        m = s ? (n_out + s - 1u) / s : 1u;
        if (m < 1) m = 1;
        t0 = t_start + ((double)s - 1.0) / (2.0 * sampling_rate);
        dt = (double)s / sampling_rate;
    }
    if (s > 0xffffffffULL) s = 0xffffffffULL;   // (one block of more than 2^32 samples: num_out is refused)
    if (m > 0xffffffffULL) throw py::value_error("hermespy_rt.compute_received_signal: more than 2^32 blocks");
    const double fc = center_frequency.is_none() ? (double)carrier_frequency * 1e9 : center_frequency.cast<double>();
    const double fa = array_frequency.is_none() ? (double)carrier_frequency * 1e9 : array_frequency.cast<double>();
    check_scene_file(mesh_filepath);
    hrt_taps_spec spec{};
    spec.fs_hz = sampling_rate; spec.fc_hz = fc; spec.t0_s = t0; spec.dt_s = dt;
    spec.l_min = (int32_t)l_min; spec.num_taps = (uint32_t)num_taps; spec.num_times = (uint32_t)m;
    spec.parts = parts_word(los, scatter);
    // (the library validates everything before it traces anything: a refused call raises ValueError.  An output
    // beyond the limits would be refused, so only one within them is allocated.)
    const bool fits = a.nr >= 1 && a.nr <= 1024 && n_out >= 1 && n_out <= (1ull << 31);
    py::array_t<std::complex<float>> out(fits ? std::vector<size_t>{(size_t)num_rx, a.nr, (size_t)2, (size_t)n_out}
                                              : std::vector<size_t>{1});
    float *dst = reinterpret_cast<float *>(out.mutable_data());
    const float *x = reinterpret_cast<const float *>(signal.data());
    const pattern_scope pattern_guard(patterns, num_rx, num_tx);
    run_pathsum("compute_received_signal", mesh_filepath, [&](Scene *scene) {
        return hrt_compute_received_signal(scene, e.rxp, e.txp, e.rxv, e.txv, carrier_frequency, num_rx, num_tx,
                                           num_paths, num_bounces, &spec, a.rxe, a.nr, a.txe, a.nt, fa, (uint32_t)s, x,
                                           (uint64_t)n, n_out, dst, nullptr);
    });
    return out;
}

// compute_beam_taps: the beamformed (codebook) sampled impulse response of the traced paths, formed on the device
// (extension; see hrt_compute_beam_taps in hermespy_rt.h): complex64 (num_rx, num_tx, Br, Bt, 2, num_times, num_taps) =
// sum_ij conj(rx_weights[a, i]) h[..., i, j, ...] tx_weights[b, j] of compute_array_taps's h, which is never formed.
py::array_t<std::complex<float>> compute_beam_taps_py(
    const std::string &mesh_filepath, farr rx_positions, farr tx_positions, farr rx_velocities, farr tx_velocities,
    float carrier_frequency, unsigned long num_rx, unsigned long num_tx, unsigned long num_paths,
    unsigned long num_bounces, double sampling_rate, unsigned long num_taps, farr rx_elements, farr tx_elements,
    py::array rx_weights, py::array tx_weights, long l_min, py::object center_frequency, double t0, double dt,
    unsigned long num_times, bool los, bool scatter, py::object array_frequency,
    py::object patterns)
{
    const endpoints e(rx_positions, tx_positions, rx_velocities, tx_velocities, num_rx, num_tx, num_paths, num_bounces);
    if (num_taps > 0xffffffffUL || num_times > 0xffffffffUL)
        throw std::invalid_argument("num_taps and num_times must fit 32 bits");
    if (l_min < -(1L << 30) || l_min > (1L << 30))
        throw py::value_error("hermespy_rt.compute_beam_taps: tap indices l_min outside +-2^24");
    const array_elements a(rx_elements, tx_elements);
    const carr wr = as_weights(rx_weights, a.nr, "rx_weights"), wt = as_weights(tx_weights, a.nt, "tx_weights");
    const size_t br = (size_t)wr.shape(0), bt = (size_t)wt.shape(0);
    const double fc = center_frequency.is_none() ? (double)carrier_frequency * 1e9 : center_frequency.cast<double>();
    const double fa = array_frequency.is_none() ? (double)carrier_frequency * 1e9 : array_frequency.cast<double>();
    check_scene_file(mesh_filepath);
    hrt_taps_spec spec{};
    spec.fs_hz = sampling_rate; spec.fc_hz = fc; spec.t0_s = t0; spec.dt_s = dt;
    spec.l_min = (int32_t)l_min; spec.num_taps = (uint32_t)num_taps; spec.num_times = (uint32_t)num_times;
    spec.parts = parts_word(los, scatter);
    // (the library validates everything before it traces anything: a refused call raises ValueError.  An output
    // beyond the limits would be refused, so only one within them is allocated.)
    const unsigned long long tl = (unsigned long long)num_times * num_taps;
    const bool fits = tl > 0 && tl <= (1ull << 20) && br <= 256 && bt <= 256 && br * bt * tl > 0 &&
                      br * bt * tl <= (1ull << 24);
    py::array_t<std::complex<float>> out(fits ? std::vector<size_t>{(size_t)num_rx, (size_t)num_tx, br, bt, (size_t)2,
                                                                    (size_t)num_times, (size_t)num_taps}
                                              : std::vector<size_t>{1});
    float *dst = reinterpret_cast<float *>(out.mutable_data());
    const float *pwr = reinterpret_cast<const float *>(wr.data()), *pwt = reinterpret_cast<const float *>(wt.data());
    const pattern_scope pattern_guard(patterns, num_rx, num_tx);
    run_pathsum("compute_beam_taps", mesh_filepath, [&](Scene *scene) {
        return hrt_compute_beam_taps(scene, e.rxp, e.txp, e.rxv, e.txv, carrier_frequency, num_rx, num_tx, num_paths,
                                     num_bounces, &spec, a.rxe, a.nr, a.txe, a.nt, fa, pwr, br, pwt, bt, dst, nullptr);
    });
    return out;
}

// compute_power_profiles: per-link power statistics of the traced paths, formed on the device (extension; see
// hrt_compute_power_profiles in hermespy_rt.h): a dict of float64 views of one flat buffer -- moments
// (num_rx, num_tx, 2, HRT_POWER_FIELDS), pdp (num_rx, num_tx, 2, Ld), arrival and departure (num_rx, num_tx, 2, Nth,
// Nph) -- and the buffer itself.
py::dict compute_power_profiles_py(
    const std::string &mesh_filepath, farr rx_positions, farr tx_positions, farr rx_velocities, farr tx_velocities,
    float carrier_frequency, unsigned long num_rx, unsigned long num_tx, unsigned long num_paths,
    unsigned long num_bounces, double tau0, double dtau, unsigned long num_delay_bins, unsigned long num_zenith_bins,
    unsigned long num_azimuth_bins, bool los, bool scatter,
    py::object patterns)
{
    const endpoints e(rx_positions, tx_positions, rx_velocities, tx_velocities, num_rx, num_tx, num_paths, num_bounces);
    if (num_delay_bins > 0xffffffffUL || num_zenith_bins > 0xffffffffUL || num_azimuth_bins > 0xffffffffUL)
        throw py::value_error("hermespy_rt.compute_power_profiles: num_delay_bins, num_zenith_bins and "
                              "num_azimuth_bins must fit 32 bits");
    check_scene_file(mesh_filepath);
    hrt_power_spec spec{};
    spec.tau0_s = tau0; spec.dtau_s = dtau;
    spec.num_delay_bins = (uint32_t)num_delay_bins;
    spec.num_zenith_bins = (uint32_t)num_zenith_bins; spec.num_azimuth_bins = (uint32_t)num_azimuth_bins;
    spec.parts = parts_word(los, scatter);
    // (the library validates the spec before it traces anything: a refused one raises ValueError; an output beyond
    // its limits is not allocated)
    const size_t links = (size_t)num_rx * num_tx, Ld = spec.num_delay_bins;
    const size_t Nth = spec.num_zenith_bins, Nph = spec.num_azimuth_bins;
    const uint64_t n = hrt_power_out_doubles(num_rx, num_tx, &spec);
    const bool fits = links <= 65535u && Ld <= (1u << 16) && Nth <= (1u << 14) && Nph <= (1u << 14) &&
                      Nth * Nph <= (1u << 14) && links * (Ld + 2u * Nth * Nph) <= (1ull << 26);
    py::array_t<double> buf(fits ? (size_t)n : (size_t)1);
    double *dst = buf.mutable_data();
    const pattern_scope pattern_guard(patterns, num_rx, num_tx);
    run_pathsum("compute_power_profiles", mesh_filepath, [&](Scene *scene) {
        return hrt_compute_power_profiles(scene, e.rxp, e.txp, e.rxv, e.txv, carrier_frequency, num_rx, num_tx, num_paths,
                                          num_bounces, &spec, dst, nullptr);
    });
    const size_t lp = links * 2u, o1 = lp * HRT_POWER_FIELDS, o2 = o1 + lp * Ld, o3 = o2 + lp * Nth * Nph;
    auto view = [&](std::vector<size_t> shape, size_t off) {
        std::vector<py::ssize_t> strides(shape.size());
        py::ssize_t st = sizeof(double);
        for (size_t k = shape.size(); k-- > 0;) {
            strides[k] = st;
            st *= (py::ssize_t)shape[k];
        }
        return py::array_t<double>(shape, strides, dst + off, buf);
    };
    const size_t R = num_rx, T = num_tx;
    py::dict d;
    d["moments"] = view({R, T, 2, (size_t)HRT_POWER_FIELDS}, 0);
    d["pdp"] = view({R, T, 2, Ld}, o1);
    d["arrival"] = view({R, T, 2, Nth, Nph}, o2);
    d["departure"] = view({R, T, 2, Nth, Nph}, o3);
    d["buffer"] = buf;
    return d;
}

// compute_array_covariance: per-link spatial covariance matrices of an antenna array, formed on the device (extension;
// see hrt_compute_array_covariance in hermespy_rt.h): a dict of complex64 views of one flat buffer -- rx (num_rx, num_tx,
// 2, Nr, Nr), tx (num_rx, num_tx, 2, Nt, Nt) -- and the buffer itself.  A side whose elements are None is not asked for
// (its view has N = 0).
py::dict compute_array_covariance_py(
    const std::string &mesh_filepath, farr rx_positions, farr tx_positions, farr rx_velocities, farr tx_velocities,
    float carrier_frequency, unsigned long num_rx, unsigned long num_tx, unsigned long num_paths,
    unsigned long num_bounces, py::object rx_elements, py::object tx_elements, bool los, bool scatter,
    py::object array_frequency,
    py::object patterns)
{
    const endpoints e(rx_positions, tx_positions, rx_velocities, tx_velocities, num_rx, num_tx, num_paths, num_bounces);
    const farr none(std::vector<size_t>{0, 3});
    const farr re = rx_elements.is_none() ? none : rx_elements.cast<farr>();
    const farr te = tx_elements.is_none() ? none : tx_elements.cast<farr>();
    const array_elements a(re, te);
    const double fa = array_frequency.is_none() ? (double)carrier_frequency * 1e9 : array_frequency.cast<double>();
    check_scene_file(mesh_filepath);
    hrt_covariance_spec spec{};
    spec.parts = parts_word(los, scatter);
    spec.sides = (rx_elements.is_none() ? 0u : HRT_COV_RX) | (tx_elements.is_none() ? 0u : HRT_COV_TX);
    // (the library validates everything before it traces anything: a refused call raises ValueError; an output beyond
    // its limits is not allocated)
    const size_t links = (size_t)num_rx * num_tx, nr = a.nr, nt = a.nt;
    const bool fits = links <= 65535u && nr <= 256u && nt <= 256u && links * 2u * (nr * nr + nt * nt) <= (1ull << 26);
    const size_t n_rx = links * 2u * nr * nr, n_tx = links * 2u * nt * nt;
    py::array_t<std::complex<float>> buf(fits ? n_rx + n_tx : (size_t)1);
    std::complex<float> *dst = buf.mutable_data();
    const pattern_scope pattern_guard(patterns, num_rx, num_tx);
    run_pathsum("compute_array_covariance", mesh_filepath, [&](Scene *scene) {
        return hrt_compute_array_covariance(scene, e.rxp, e.txp, e.rxv, e.txv, carrier_frequency, num_rx, num_tx,
                                            num_paths, num_bounces, &spec, a.rxe, a.nr, a.txe, a.nt, fa,
                                            reinterpret_cast<float *>(dst), nullptr);
    });
    auto view = [&](size_t n, size_t off) {
        const std::vector<size_t> shape{(size_t)num_rx, (size_t)num_tx, 2, n, n};
        std::vector<py::ssize_t> strides(shape.size());
        py::ssize_t st = sizeof(std::complex<float>);
        for (size_t k = shape.size(); k-- > 0;) {
            strides[k] = st;
            st *= (py::ssize_t)shape[k];
        }
        return py::array_t<std::complex<float>>(shape, strides, dst + off, buf);
    };
    py::dict d;
    d["rx"] = view(nr, 0);
    d["tx"] = view(nt, n_rx);
    d["buffer"] = buf;
    return d;
}

// the views of a dominant paths buffer (hrt_dominant_out_bytes = n bytes at dst, kept alive by `buf`) as a dict:
// compute_dominant_paths' result, and compute_sparse_array_channel's lists
py::dict dominant_dict(py::array_t<uint64_t> &buf, uint8_t *dst, uint64_t n, unsigned long num_rx, unsigned long num_tx,
                       unsigned long max_paths)
{
    const py::ssize_t R = (py::ssize_t)num_rx, T = (py::ssize_t)num_tx, K = (py::ssize_t)max_paths;
    const py::ssize_t rec = (py::ssize_t)sizeof(hrt_dominant_path);
    uint8_t *recs = dst + 16 * R * T;
    auto field = [&](auto *proto, size_t off) {
        using V = std::remove_pointer_t<decltype(proto)>;
        return py::array_t<V>({R, T, K}, {T * K * rec, K * rec, rec}, reinterpret_cast<V *>(recs + off), buf);
    };
    auto vec3 = [&](size_t off) {
        return py::array_t<float>({R, T, K, (py::ssize_t)3}, {T * K * rec, K * rec, rec, (py::ssize_t)4},
                                  reinterpret_cast<float *>(recs + off), buf);
    };
    auto header = [&](size_t word) {
        return py::array_t<uint64_t>({R, T}, {T * 16, (py::ssize_t)16}, reinterpret_cast<uint64_t *>(dst) + word, buf);
    };
    py::dict d;
    d["kept"] = header(0);
    d["eligible"] = header(1);
    d["power"] = field((double *)nullptr, offsetof(hrt_dominant_path, power));
    d["path"] = field((uint64_t *)nullptr, offsetof(hrt_dominant_path, path));
    d["bounce"] = field((int32_t *)nullptr, offsetof(hrt_dominant_path, bounce));
    d["tri"] = field((uint32_t *)nullptr, offsetof(hrt_dominant_path, tri));
    d["a_te"] = field((std::complex<float> *)nullptr, offsetof(hrt_dominant_path, a_te_re));
    d["a_tm"] = field((std::complex<float> *)nullptr, offsetof(hrt_dominant_path, a_tm_re));
    d["tau"] = field((float *)nullptr, offsetof(hrt_dominant_path, tau));
    d["freq_shift"] = field((float *)nullptr, offsetof(hrt_dominant_path, freq_shift));
    d["u_rx"] = vec3(offsetof(hrt_dominant_path, u_rx));
    d["u_tx"] = vec3(offsetof(hrt_dominant_path, u_tx));
    d["buffer"] = py::array_t<uint8_t>({(py::ssize_t)n}, {(py::ssize_t)1}, dst, buf);
    return d;
}

// compute_dominant_paths: the max_paths strongest paths of every link, selected on the device (extension; see
// hrt_compute_dominant_paths in hermespy_rt.h): a dict of views of one buffer -- kept, eligible (num_rx, num_tx);
// power, path, bounce, tri, tau, freq_shift (num_rx, num_tx, K); a_te, a_tm complex64 (num_rx, num_tx, K); u_rx, u_tx
// (num_rx, num_tx, K, 3) -- and the buffer itself (uint8).
py::dict compute_dominant_paths_py(
    const std::string &mesh_filepath, farr rx_positions, farr tx_positions, farr rx_velocities, farr tx_velocities,
    float carrier_frequency, unsigned long num_rx, unsigned long num_tx, unsigned long num_paths,
    unsigned long num_bounces, unsigned long max_paths, bool los, bool scatter,
    py::object patterns)
{
    const endpoints e(rx_positions, tx_positions, rx_velocities, tx_velocities, num_rx, num_tx, num_paths, num_bounces);
    if (max_paths > 0xffffffffUL)
        throw py::value_error("hermespy_rt.compute_dominant_paths: max_paths must fit 32 bits");
    check_scene_file(mesh_filepath);
    hrt_dominant_spec spec{};
    spec.max_paths = (uint32_t)max_paths;
    spec.parts = parts_word(los, scatter);
    // (the library validates the spec before it traces anything: a refused one raises ValueError and has no output)
    const uint64_t n = hrt_dominant_out_bytes(num_rx, num_tx, &spec);
    py::array_t<uint64_t> buf((size_t)(n ? n / 8u : 1u));   // (8-byte aligned words; 72 and 16 are multiples of 8)
    uint8_t *dst = reinterpret_cast<uint8_t *>(buf.mutable_data());
    const pattern_scope pattern_guard(patterns, num_rx, num_tx);
    run_pathsum("compute_dominant_paths", mesh_filepath, [&](Scene *scene) {
        return hrt_compute_dominant_paths(scene, e.rxp, e.txp, e.rxv, e.txv, carrier_frequency, num_rx, num_tx,
                                          num_paths, num_bounces, &spec, dst, nullptr);
    });
    return dominant_dict(buf, dst, n, num_rx, num_tx, max_paths);
}

// compute_sparse_array_channel: the antenna-array channel of the max_paths strongest paths of every link, selected and
// evaluated on the device (extension; see hrt_compute_sparse_array_channel in hermespy_rt.h): complex64 (num_rx, num_tx,
// Nr, Nt, 2, num_times, num_freqs), or with return_paths the tuple (H, compute_dominant_paths' dict of the lists).
py::object compute_sparse_array_channel_py(
    const std::string &mesh_filepath, farr rx_positions, farr tx_positions, farr rx_velocities, farr tx_velocities,
    float carrier_frequency, unsigned long num_rx, unsigned long num_tx, unsigned long num_paths,
    unsigned long num_bounces, double f0, double df, unsigned long num_freqs, farr rx_elements, farr tx_elements,
    unsigned long max_paths, double t0, double dt, unsigned long num_times, bool los, bool scatter,
    py::object array_frequency, py::object patterns, bool return_paths)
{
    const endpoints e(rx_positions, tx_positions, rx_velocities, tx_velocities, num_rx, num_tx, num_paths, num_bounces);
    if (num_freqs > 0xffffffffUL || num_times > 0xffffffffUL)
        throw std::invalid_argument("num_freqs and num_times must fit 32 bits");
    if (max_paths > 0xffffffffUL)
        throw py::value_error("hermespy_rt.compute_sparse_array_channel: max_paths must fit 32 bits");
    const array_elements a(rx_elements, tx_elements);
    const double fa = array_frequency.is_none() ? (double)carrier_frequency * 1e9 : array_frequency.cast<double>();
    check_scene_file(mesh_filepath);
    hrt_dominant_spec dm{};
    dm.max_paths = (uint32_t)max_paths;
    dm.parts = parts_word(los, scatter);
    hrt_channel_spec grid{};
    grid.f0_hz = f0; grid.df_hz = df; grid.num_freqs = (uint32_t)num_freqs;
    grid.t0_s = t0; grid.dt_s = dt; grid.num_times = (uint32_t)num_times;
    grid.parts = dm.parts;
    // (the library validates everything before it traces anything: a refused call raises ValueError.  Outputs beyond
    // the limits would be refused, so only ones within them are allocated.)
    const uint64_t n = hrt_dominant_out_bytes(num_rx, num_tx, &dm);
    const bool fits = n && a.fits((unsigned long long)num_times * num_freqs);
    py::array_t<std::complex<float>> out(fits ? std::vector<size_t>{(size_t)num_rx, (size_t)num_tx, a.nr, a.nt, (size_t)2,
                                                                    (size_t)num_times, (size_t)num_freqs}
                                              : std::vector<size_t>{1});
    float *dst = reinterpret_cast<float *>(out.mutable_data());
    py::array_t<uint64_t> buf((size_t)(return_paths && n ? n / 8u : 1u));
    uint8_t *lists = reinterpret_cast<uint8_t *>(buf.mutable_data());
    const pattern_scope pattern_guard(patterns, num_rx, num_tx);
    run_pathsum("compute_sparse_array_channel", mesh_filepath, [&](Scene *scene) {
        return hrt_compute_sparse_array_channel(scene, e.rxp, e.txp, e.rxv, e.txv, carrier_frequency, num_rx, num_tx,
                                                num_paths, num_bounces, &dm, &grid, a.rxe, a.nr, a.txe, a.nt, fa, dst,
                                                return_paths ? (void *)lists : nullptr, nullptr);
    });
    if (!return_paths) return out;
    return py::make_tuple(out, dominant_dict(buf, lists, n, num_rx, num_tx, max_paths));
}

// compute_sparse_beam_channel: the beamformed (codebook) channel of the max_paths strongest paths of every link,
// selected and evaluated on the device (extension; see hrt_compute_sparse_beam_channel in hermespy_rt.h): complex64
// (num_rx, num_tx, Br, Bt, 2, num_times, num_freqs), or with return_paths the tuple (B, compute_dominant_paths' dict of
// the lists).  rx_weights (Br, Nr) is applied conjugated, tx_weights (Bt, Nt) as it is.
py::object compute_sparse_beam_channel_py(
    const std::string &mesh_filepath, farr rx_positions, farr tx_positions, farr rx_velocities, farr tx_velocities,
    float carrier_frequency, unsigned long num_rx, unsigned long num_tx, unsigned long num_paths,
    unsigned long num_bounces, double f0, double df, unsigned long num_freqs, farr rx_elements, farr tx_elements,
    py::array rx_weights, py::array tx_weights, unsigned long max_paths, double t0, double dt, unsigned long num_times,
    bool los, bool scatter, py::object array_frequency, py::object patterns, bool return_paths)
{
    const endpoints e(rx_positions, tx_positions, rx_velocities, tx_velocities, num_rx, num_tx, num_paths, num_bounces);
    if (num_freqs > 0xffffffffUL || num_times > 0xffffffffUL)
        throw std::invalid_argument("num_freqs and num_times must fit 32 bits");
    if (max_paths > 0xffffffffUL)
        throw py::value_error("hermespy_rt.compute_sparse_beam_channel: max_paths must fit 32 bits");
    const array_elements a(rx_elements, tx_elements);
    const carr wr = as_weights(rx_weights, a.nr, "rx_weights"), wt = as_weights(tx_weights, a.nt, "tx_weights");
    const size_t br = (size_t)wr.shape(0), bt = (size_t)wt.shape(0);
    const double fa = array_frequency.is_none() ? (double)carrier_frequency * 1e9 : array_frequency.cast<double>();
    check_scene_file(mesh_filepath);
    hrt_dominant_spec dm{};
    dm.max_paths = (uint32_t)max_paths;
    dm.parts = parts_word(los, scatter);
    hrt_channel_spec grid{};
    grid.f0_hz = f0; grid.df_hz = df; grid.num_freqs = (uint32_t)num_freqs;
    grid.t0_s = t0; grid.dt_s = dt; grid.num_times = (uint32_t)num_times;
    grid.parts = dm.parts;
    // (the library validates everything before it traces anything: a refused call raises ValueError.  Outputs beyond
    // the limits would be refused, so only ones within them are allocated.)
    const uint64_t n = hrt_dominant_out_bytes(num_rx, num_tx, &dm);
    const unsigned long long pts = (unsigned long long)br * bt * num_times * num_freqs;
    const bool fits = n && pts > 0 && pts <= (1ull << 24) && br <= 256 && bt <= 256;
    py::array_t<std::complex<float>> out(fits ? std::vector<size_t>{(size_t)num_rx, (size_t)num_tx, br, bt, (size_t)2,
                                                                    (size_t)num_times, (size_t)num_freqs}
                                              : std::vector<size_t>{1});
    float *dst = reinterpret_cast<float *>(out.mutable_data());
    const float *pwr = reinterpret_cast<const float *>(wr.data()), *pwt = reinterpret_cast<const float *>(wt.data());
    py::array_t<uint64_t> buf((size_t)(return_paths && n ? n / 8u : 1u));
    uint8_t *lists = reinterpret_cast<uint8_t *>(buf.mutable_data());
    const pattern_scope pattern_guard(patterns, num_rx, num_tx);
    run_pathsum("compute_sparse_beam_channel", mesh_filepath, [&](Scene *scene) {
        return hrt_compute_sparse_beam_channel(scene, e.rxp, e.txp, e.rxv, e.txv, carrier_frequency, num_rx, num_tx,
                                               num_paths, num_bounces, &dm, &grid, a.rxe, a.nr, a.txe, a.nt, fa, pwr, br,
                                               pwt, bt, dst, return_paths ? (void *)lists : nullptr, nullptr);
    });
    if (!return_paths) return out;
    return py::make_tuple(out, dominant_dict(buf, lists, n, num_rx, num_tx, max_paths));
}

// compute_sparse_array_taps: the antenna-array impulse responses of the max_paths strongest paths of every link,
// selected and evaluated on the device (extension; see hrt_compute_sparse_array_taps in hermespy_rt.h): complex64
// (num_rx, num_tx, Nr, Nt, 2, num_times, num_taps), or with return_paths the tuple (h, compute_dominant_paths' dict of
// the lists).
py::object compute_sparse_array_taps_py(
    const std::string &mesh_filepath, farr rx_positions, farr tx_positions, farr rx_velocities, farr tx_velocities,
    float carrier_frequency, unsigned long num_rx, unsigned long num_tx, unsigned long num_paths,
    unsigned long num_bounces, double sampling_rate, unsigned long num_taps, farr rx_elements, farr tx_elements,
    unsigned long max_paths, long l_min, py::object center_frequency, double t0, double dt, unsigned long num_times,
    bool los, bool scatter, py::object array_frequency, py::object patterns, bool return_paths)
{
    const endpoints e(rx_positions, tx_positions, rx_velocities, tx_velocities, num_rx, num_tx, num_paths, num_bounces);
    if (num_taps > 0xffffffffUL || num_times > 0xffffffffUL)
        throw std::invalid_argument("num_taps and num_times must fit 32 bits");
    if (l_min < -(1L << 30) || l_min > (1L << 30))
        throw py::value_error("hermespy_rt.compute_sparse_array_taps: tap indices l_min outside +-2^24");
    if (max_paths > 0xffffffffUL)
        throw py::value_error("hermespy_rt.compute_sparse_array_taps: max_paths must fit 32 bits");
    const array_elements a(rx_elements, tx_elements);
    const double fc = center_frequency.is_none() ? (double)carrier_frequency * 1e9 : center_frequency.cast<double>();
    const double fa = array_frequency.is_none() ? (double)carrier_frequency * 1e9 : array_frequency.cast<double>();
    check_scene_file(mesh_filepath);
    hrt_dominant_spec dm{};
    dm.max_paths = (uint32_t)max_paths;
    dm.parts = parts_word(los, scatter);
    hrt_taps_spec grid{};
    grid.fs_hz = sampling_rate; grid.fc_hz = fc; grid.t0_s = t0; grid.dt_s = dt;
    grid.l_min = (int32_t)l_min; grid.num_taps = (uint32_t)num_taps; grid.num_times = (uint32_t)num_times;
    grid.parts = dm.parts;
    // (the library validates everything before it traces anything: a refused call raises ValueError.  Outputs beyond
    // the limits would be refused, so only ones within them are allocated.)
    const uint64_t n = hrt_dominant_out_bytes(num_rx, num_tx, &dm);
    const bool fits = n && a.fits((unsigned long long)num_times * num_taps) &&
                      (uint64_t)num_taps * num_times <= (1ull << 20);
    py::array_t<std::complex<float>> out(fits ? std::vector<size_t>{(size_t)num_rx, (size_t)num_tx, a.nr, a.nt, (size_t)2,
                                                                    (size_t)num_times, (size_t)num_taps}
                                              : std::vector<size_t>{1});
    float *dst = reinterpret_cast<float *>(out.mutable_data());
    py::array_t<uint64_t> buf((size_t)(return_paths && n ? n / 8u : 1u));
    uint8_t *lists = reinterpret_cast<uint8_t *>(buf.mutable_data());
    const pattern_scope pattern_guard(patterns, num_rx, num_tx);
    run_pathsum("compute_sparse_array_taps", mesh_filepath, [&](Scene *scene) {
        return hrt_compute_sparse_array_taps(scene, e.rxp, e.txp, e.rxv, e.txv, carrier_frequency, num_rx, num_tx,
                                             num_paths, num_bounces, &dm, &grid, a.rxe, a.nr, a.txe, a.nt, fa, dst,
                                             return_paths ? (void *)lists : nullptr, nullptr);
    });
    if (!return_paths) return out;
    return py::make_tuple(out, dominant_dict(buf, lists, n, num_rx, num_tx, max_paths));
}

// compute_sparse_beam_taps: the beamformed (codebook) impulse responses of the max_paths strongest paths of every link,
// selected and evaluated on the device (extension; see hrt_compute_sparse_beam_taps in hermespy_rt.h): complex64
// (num_rx, num_tx, Br, Bt, 2, num_times, num_taps), or with return_paths the tuple (h, compute_dominant_paths' dict of
// the lists).  rx_weights (Br, Nr) is applied conjugated, tx_weights (Bt, Nt) as it is.
py::object compute_sparse_beam_taps_py(
    const std::string &mesh_filepath, farr rx_positions, farr tx_positions, farr rx_velocities, farr tx_velocities,
    float carrier_frequency, unsigned long num_rx, unsigned long num_tx, unsigned long num_paths,
    unsigned long num_bounces, double sampling_rate, unsigned long num_taps, farr rx_elements, farr tx_elements,
    py::array rx_weights, py::array tx_weights, unsigned long max_paths, long l_min, py::object center_frequency,
    double t0, double dt, unsigned long num_times, bool los, bool scatter, py::object array_frequency,
    py::object patterns, bool return_paths)
{
    const endpoints e(rx_positions, tx_positions, rx_velocities, tx_velocities, num_rx, num_tx, num_paths, num_bounces);
    if (num_taps > 0xffffffffUL || num_times > 0xffffffffUL)
        throw std::invalid_argument("num_taps and num_times must fit 32 bits");
    if (l_min < -(1L << 30) || l_min > (1L << 30))
        throw py::value_error("hermespy_rt.compute_sparse_beam_taps: tap indices l_min outside +-2^24");
    if (max_paths > 0xffffffffUL)
        throw py::value_error("hermespy_rt.compute_sparse_beam_taps: max_paths must fit 32 bits");
    const array_elements a(rx_elements, tx_elements);
    const carr wr = as_weights(rx_weights, a.nr, "rx_weights"), wt = as_weights(tx_weights, a.nt, "tx_weights");
    const size_t br = (size_t)wr.shape(0), bt = (size_t)wt.shape(0);
    const double fc = center_frequency.is_none() ? (double)carrier_frequency * 1e9 : center_frequency.cast<double>();
    const double fa = array_frequency.is_none() ? (double)carrier_frequency * 1e9 : array_frequency.cast<double>();
    check_scene_file(mesh_filepath);
    hrt_dominant_spec dm{};
    dm.max_paths = (uint32_t)max_paths;
    dm.parts = parts_word(los, scatter);
    hrt_taps_spec grid{};
    grid.fs_hz = sampling_rate; grid.fc_hz = fc; grid.t0_s = t0; grid.dt_s = dt;
    grid.l_min = (int32_t)l_min; grid.num_taps = (uint32_t)num_taps; grid.num_times = (uint32_t)num_times;
    grid.parts = dm.parts;
    // (the library validates everything before it traces anything: a refused call raises ValueError.  Outputs beyond
    // the limits would be refused, so only ones within them are allocated.)
    const uint64_t n = hrt_dominant_out_bytes(num_rx, num_tx, &dm);
    const unsigned long long pts = (unsigned long long)br * bt * num_times * num_taps;
    const bool fits = n && pts > 0 && pts <= (1ull << 24) && br <= 256 && bt <= 256 &&
                      (uint64_t)num_taps * num_times <= (1ull << 20);
    py::array_t<std::complex<float>> out(fits ? std::vector<size_t>{(size_t)num_rx, (size_t)num_tx, br, bt, (size_t)2,
                                                                    (size_t)num_times, (size_t)num_taps}
                                              : std::vector<size_t>{1});
    float *dst = reinterpret_cast<float *>(out.mutable_data());
    const float *pwr = reinterpret_cast<const float *>(wr.data()), *pwt = reinterpret_cast<const float *>(wt.data());
    py::array_t<uint64_t> buf((size_t)(return_paths && n ? n / 8u : 1u));
    uint8_t *lists = reinterpret_cast<uint8_t *>(buf.mutable_data());
    const pattern_scope pattern_guard(patterns, num_rx, num_tx);
    run_pathsum("compute_sparse_beam_taps", mesh_filepath, [&](Scene *scene) {
        return hrt_compute_sparse_beam_taps(scene, e.rxp, e.txp, e.rxv, e.txv, carrier_frequency, num_rx, num_tx,
                                            num_paths, num_bounces, &dm, &grid, a.rxe, a.nr, a.txe, a.nt, fa, pwr, br,
                                            pwt, bt, dst, return_paths ? (void *)lists : nullptr, nullptr);
    });
    if (!return_paths) return out;
    return py::make_tuple(out, dominant_dict(buf, lists, n, num_rx, num_tx, max_paths));
}

}  // namespace

PYBIND11_MODULE(hermespy_rt, m)
{
    m.doc() = "MI355X-native compute_paths (drop-in for the hermespy-rt binding)";
    py::class_<ChannelInfoPy>(m, "ChannelInfo")
        .def_readonly("num_paths", &ChannelInfoPy::num_paths)
        .def_readonly("directions_rx", &ChannelInfoPy::directions_rx)
        .def_readonly("directions_tx", &ChannelInfoPy::directions_tx)
        .def_readonly("a_te", &ChannelInfoPy::a_te)
        .def_readonly("a_tm", &ChannelInfoPy::a_tm)
        .def_readonly("tau", &ChannelInfoPy::tau)
        .def_readonly("freq_shift", &ChannelInfoPy::freq_shift);
    m.def("compute_paths", &compute_paths_py, "Compute gains and delays",
          py::arg("mesh_filepath"), py::arg("rx_positions"), py::arg("tx_positions"),
          py::arg("rx_velocities"), py::arg("tx_velocities"), py::arg("carrier_frequency"),
          py::arg("num_rx"), py::arg("num_tx"), py::arg("num_paths"), py::arg("num_bounces"));
    m.def("compute_paths_list", &compute_paths_list_py,
          "compute_paths with the result as one list of path records (dict of arrays)",
          py::arg("mesh_filepath"), py::arg("rx_positions"), py::arg("tx_positions"),
          py::arg("rx_velocities"), py::arg("tx_velocities"), py::arg("carrier_frequency"),
          py::arg("num_rx"), py::arg("num_tx"), py::arg("num_paths"), py::arg("num_bounces"),
          py::arg("include_blocked") = false);
    m.def("compute_channel", &compute_channel_py,
          "Channel frequency response of the traced paths, formed on the device: complex64 "
          "(num_rx, num_tx, 2, num_times, num_freqs)",
          py::arg("mesh_filepath"), py::arg("rx_positions"), py::arg("tx_positions"),
          py::arg("rx_velocities"), py::arg("tx_velocities"), py::arg("carrier_frequency"),
          py::arg("num_rx"), py::arg("num_tx"), py::arg("num_paths"), py::arg("num_bounces"),
          py::arg("f0"), py::arg("df"), py::arg("num_freqs"), py::arg("t0") = 0.0, py::arg("dt") = 0.0,
          py::arg("num_times") = 1, py::arg("los") = true, py::arg("scatter") = true,
          py::arg("patterns") = py::none());
    m.def("compute_array_channel", &compute_array_channel_py,
          "Antenna-array channel of the traced paths, formed on the device: complex64 "
          "(num_rx, num_tx, Nr, Nt, 2, num_times, num_freqs)",
          py::arg("mesh_filepath"), py::arg("rx_positions"), py::arg("tx_positions"),
          py::arg("rx_velocities"), py::arg("tx_velocities"), py::arg("carrier_frequency"),
          py::arg("num_rx"), py::arg("num_tx"), py::arg("num_paths"), py::arg("num_bounces"),
          py::arg("f0"), py::arg("df"), py::arg("num_freqs"), py::arg("rx_elements"), py::arg("tx_elements"),
          py::arg("t0") = 0.0, py::arg("dt") = 0.0, py::arg("num_times") = 1, py::arg("los") = true,
          py::arg("scatter") = true, py::arg("array_frequency") = py::none(), py::arg("patterns") = py::none());
    m.def("compute_channel_svd", &compute_channel_svd_py,
          "Per-point MIMO SVD of the antenna-array channel, formed on the device: a dict of views of one buffer -- "
          "sigma (num_rx, num_tx, n, 2, num_times, num_freqs), u (.., Nr, n, ..), v (.., Nt, n, ..), sweeps, buffer",
          py::arg("mesh_filepath"), py::arg("rx_positions"), py::arg("tx_positions"),
          py::arg("rx_velocities"), py::arg("tx_velocities"), py::arg("carrier_frequency"),
          py::arg("num_rx"), py::arg("num_tx"), py::arg("num_paths"), py::arg("num_bounces"),
          py::arg("f0"), py::arg("df"), py::arg("num_freqs"), py::arg("rx_elements"), py::arg("tx_elements"),
          py::arg("t0") = 0.0, py::arg("dt") = 0.0, py::arg("num_times") = 1, py::arg("los") = true,
          py::arg("scatter") = true, py::arg("array_frequency") = py::none(), py::arg("vectors") = true,
          py::arg("patterns") = py::none());
    m.def("compute_channel_equalizer", &compute_channel_equalizer_py,
          "Per-point linear MIMO equalizer (kind 'zf' or 'lmmse') of the antenna-array channel and its SINR, formed on "
          "the device: a dict of views of one buffer -- W (num_rx, num_tx, Nt, Nr, 2, num_times, num_freqs), "
          "sinr (.., Nt, 2, ..), status, buffer",
          py::arg("mesh_filepath"), py::arg("rx_positions"), py::arg("tx_positions"),
          py::arg("rx_velocities"), py::arg("tx_velocities"), py::arg("carrier_frequency"),
          py::arg("num_rx"), py::arg("num_tx"), py::arg("num_paths"), py::arg("num_bounces"),
          py::arg("f0"), py::arg("df"), py::arg("num_freqs"), py::arg("rx_elements"), py::arg("tx_elements"),
          py::arg("noise"), py::arg("kind") = "lmmse", py::arg("t0") = 0.0, py::arg("dt") = 0.0,
          py::arg("num_times") = 1, py::arg("los") = true, py::arg("scatter") = true,
          py::arg("array_frequency") = py::none(), py::arg("weights") = true, py::arg("patterns") = py::none());
    m.def("compute_channel_precoder", &compute_channel_precoder_py,
          "Per-point linear MIMO precoder (kind 'mrt', 'zf' or 'rzf'; normalize 'total' or 'stream') of the "
          "antenna-array channel and the downlink SINR behind it, formed on the device: a dict of views of one buffer "
          "-- P (num_rx, num_tx, Nt, Nr, 2, num_times, num_freqs), sinr (.., Nr, 2, ..), status, buffer",
          py::arg("mesh_filepath"), py::arg("rx_positions"), py::arg("tx_positions"),
          py::arg("rx_velocities"), py::arg("tx_velocities"), py::arg("carrier_frequency"),
          py::arg("num_rx"), py::arg("num_tx"), py::arg("num_paths"), py::arg("num_bounces"),
          py::arg("f0"), py::arg("df"), py::arg("num_freqs"), py::arg("rx_elements"), py::arg("tx_elements"),
          py::arg("noise"), py::arg("kind") = "rzf", py::arg("power") = 1.0f, py::arg("regularization") = py::none(),
          py::arg("normalize") = "total", py::arg("t0") = 0.0, py::arg("dt") = 0.0, py::arg("num_times") = 1,
          py::arg("los") = true, py::arg("scatter") = true, py::arg("array_frequency") = py::none(),
          py::arg("weights") = true, py::arg("patterns") = py::none());
    m.def("compute_codebook_select", &compute_codebook_select_py,
          "Per-subband precoder codebook selection (metric 'power' or 'capacity') on the antenna-array channel, formed "
          "on the device: a dict of views of one buffer -- index, metric, status (num_rx, num_tx, 2, num_times, B), "
          "table (num_rx, num_tx, C, 2, num_times, B), effective (num_rx, num_tx, Nr, L, 2, num_times, num_freqs), buffer",
          py::arg("mesh_filepath"), py::arg("rx_positions"), py::arg("tx_positions"),
          py::arg("rx_velocities"), py::arg("tx_velocities"), py::arg("carrier_frequency"),
          py::arg("num_rx"), py::arg("num_tx"), py::arg("num_paths"), py::arg("num_bounces"),
          py::arg("f0"), py::arg("df"), py::arg("num_freqs"), py::arg("rx_elements"), py::arg("tx_elements"),
          py::arg("codebook"), py::arg("metric") = "capacity", py::arg("noise") = py::none(),
          py::arg("subband") = py::none(), py::arg("t0") = 0.0, py::arg("dt") = 0.0, py::arg("num_times") = 1,
          py::arg("los") = true, py::arg("scatter") = true, py::arg("array_frequency") = py::none(),
          py::arg("table") = false, py::arg("effective") = false, py::arg("patterns") = py::none());
    m.def("compute_channel_detect", &compute_channel_detect_py,
          "Per-point maximum-likelihood MIMO detection with max-log bit LLRs on the antenna-array channel, formed on "
          "the device: a dict of views of one buffer -- index, metric, status (num_rx, num_tx, 2, num_times, num_freqs), "
          "llr (num_rx, num_tx, Nt, B, 2, num_times, num_freqs), buffer",
          py::arg("mesh_filepath"), py::arg("rx_positions"), py::arg("tx_positions"),
          py::arg("rx_velocities"), py::arg("tx_velocities"), py::arg("carrier_frequency"),
          py::arg("num_rx"), py::arg("num_tx"), py::arg("num_paths"), py::arg("num_bounces"),
          py::arg("f0"), py::arg("df"), py::arg("num_freqs"), py::arg("rx_elements"), py::arg("tx_elements"),
          py::arg("Y"), py::arg("constellation"), py::arg("noise"), py::arg("t0") = 0.0, py::arg("dt") = 0.0,
          py::arg("num_times") = 1, py::arg("los") = true, py::arg("scatter") = true,
          py::arg("array_frequency") = py::none(), py::arg("llr") = true, py::arg("patterns") = py::none());
    m.def("compute_channel_kbest", &compute_channel_kbest_py,
          "Per-point K-best tree-search MIMO detection with list max-log bit LLRs on the antenna-array channel, formed "
          "on the device: a dict of views of one buffer -- index, metric, status (num_rx, num_tx, 2, num_times, "
          "num_freqs), llr (num_rx, num_tx, Nt, B, 2, num_times, num_freqs), buffer",
          py::arg("mesh_filepath"), py::arg("rx_positions"), py::arg("tx_positions"),
          py::arg("rx_velocities"), py::arg("tx_velocities"), py::arg("carrier_frequency"),
          py::arg("num_rx"), py::arg("num_tx"), py::arg("num_paths"), py::arg("num_bounces"),
          py::arg("f0"), py::arg("df"), py::arg("num_freqs"), py::arg("rx_elements"), py::arg("tx_elements"),
          py::arg("Y"), py::arg("constellation"), py::arg("noise"), py::arg("k"), py::arg("clip"),
          py::arg("t0") = 0.0, py::arg("dt") = 0.0, py::arg("num_times") = 1, py::arg("los") = true,
          py::arg("scatter") = true, py::arg("array_frequency") = py::none(), py::arg("sorted") = true,
          py::arg("llr") = true, py::arg("patterns") = py::none());
    m.def("compute_beam_channel", &compute_beam_channel_py,
          "Beamformed (codebook) channel of the traced paths, formed on the device: complex64 "
          "(num_rx, num_tx, Br, Bt, 2, num_times, num_freqs); rx_weights (Br, Nr) is applied conjugated, tx_weights "
          "(Bt, Nt) as it is",
          py::arg("mesh_filepath"), py::arg("rx_positions"), py::arg("tx_positions"),
          py::arg("rx_velocities"), py::arg("tx_velocities"), py::arg("carrier_frequency"),
          py::arg("num_rx"), py::arg("num_tx"), py::arg("num_paths"), py::arg("num_bounces"),
          py::arg("f0"), py::arg("df"), py::arg("num_freqs"), py::arg("rx_elements"), py::arg("tx_elements"),
          py::arg("rx_weights"), py::arg("tx_weights"), py::arg("t0") = 0.0, py::arg("dt") = 0.0,
          py::arg("num_times") = 1, py::arg("los") = true, py::arg("scatter") = true,
          py::arg("array_frequency") = py::none(), py::arg("patterns") = py::none());
    m.def("compute_taps", &compute_taps_py,
          "Sampled channel impulse response of the traced paths, formed on the device: complex64 "
          "(num_rx, num_tx, 2, num_times, num_taps)",
          py::arg("mesh_filepath"), py::arg("rx_positions"), py::arg("tx_positions"),
          py::arg("rx_velocities"), py::arg("tx_velocities"), py::arg("carrier_frequency"),
          py::arg("num_rx"), py::arg("num_tx"), py::arg("num_paths"), py::arg("num_bounces"),
          py::arg("sampling_rate"), py::arg("num_taps"), py::arg("l_min") = 0,
          py::arg("center_frequency") = py::none(), py::arg("t0") = 0.0, py::arg("dt") = 0.0,
          py::arg("num_times") = 1, py::arg("los") = true, py::arg("scatter") = true,
          py::arg("patterns") = py::none());
    m.def("compute_array_taps", &compute_array_taps_py,
          "Antenna-array sampled channel impulse response of the traced paths, formed on the device: complex64 "
          "(num_rx, num_tx, Nr, Nt, 2, num_times, num_taps)",
          py::arg("mesh_filepath"), py::arg("rx_positions"), py::arg("tx_positions"),
          py::arg("rx_velocities"), py::arg("tx_velocities"), py::arg("carrier_frequency"),
          py::arg("num_rx"), py::arg("num_tx"), py::arg("num_paths"), py::arg("num_bounces"),
          py::arg("sampling_rate"), py::arg("num_taps"), py::arg("rx_elements"), py::arg("tx_elements"),
          py::arg("l_min") = 0, py::arg("center_frequency") = py::none(), py::arg("t0") = 0.0, py::arg("dt") = 0.0,
          py::arg("num_times") = 1, py::arg("los") = true, py::arg("scatter") = true,
          py::arg("array_frequency") = py::none(), py::arg("patterns") = py::none());
    m.def("compute_received_signal", &compute_received_signal_py,
          "The samples the receivers see when the transmitters send `signal` (num_tx, Nt, N) through the traced "
          "channel, formed on the device: complex64 (num_rx, Nr, 2, num_out)",
          py::arg("mesh_filepath"), py::arg("rx_positions"), py::arg("tx_positions"),
          py::arg("rx_velocities"), py::arg("tx_velocities"), py::arg("carrier_frequency"),
          py::arg("num_rx"), py::arg("num_tx"), py::arg("num_paths"), py::arg("num_bounces"),
          py::arg("sampling_rate"), py::arg("num_taps"), py::arg("rx_elements"), py::arg("tx_elements"),
          py::arg("signal"), py::arg("l_min") = 0, py::arg("samples_per_block") = py::none(),
          py::arg("t_start") = 0.0, py::arg("center_frequency") = py::none(), py::arg("num_out") = py::none(),
          py::arg("los") = true, py::arg("scatter") = true, py::arg("array_frequency") = py::none(), py::arg("patterns") = py::none());
    m.def("compute_beam_taps", &compute_beam_taps_py,
          "Beamformed (codebook) sampled channel impulse response of the traced paths, formed on the device: complex64 "
          "(num_rx, num_tx, Br, Bt, 2, num_times, num_taps); rx_weights (Br, Nr) is applied conjugated, tx_weights "
          "(Bt, Nt) as it is",
          py::arg("mesh_filepath"), py::arg("rx_positions"), py::arg("tx_positions"),
          py::arg("rx_velocities"), py::arg("tx_velocities"), py::arg("carrier_frequency"),
          py::arg("num_rx"), py::arg("num_tx"), py::arg("num_paths"), py::arg("num_bounces"),
          py::arg("sampling_rate"), py::arg("num_taps"), py::arg("rx_elements"), py::arg("tx_elements"),
          py::arg("rx_weights"), py::arg("tx_weights"), py::arg("l_min") = 0,
          py::arg("center_frequency") = py::none(), py::arg("t0") = 0.0, py::arg("dt") = 0.0,
          py::arg("num_times") = 1, py::arg("los") = true, py::arg("scatter") = true,
          py::arg("array_frequency") = py::none(), py::arg("patterns") = py::none());
    m.def("compute_power_profiles", &compute_power_profiles_py,
          "Per-link power statistics of the traced paths, formed on the device: a dict of float64 arrays "
          "(moments, pdp, arrival, departure, buffer)",
          py::arg("mesh_filepath"), py::arg("rx_positions"), py::arg("tx_positions"),
          py::arg("rx_velocities"), py::arg("tx_velocities"), py::arg("carrier_frequency"),
          py::arg("num_rx"), py::arg("num_tx"), py::arg("num_paths"), py::arg("num_bounces"),
          py::arg("tau0"), py::arg("dtau"), py::arg("num_delay_bins"), py::arg("num_zenith_bins") = 0,
          py::arg("num_azimuth_bins") = 0, py::arg("los") = true, py::arg("scatter") = true,
          py::arg("patterns") = py::none());
    m.def("compute_array_covariance", &compute_array_covariance_py,
          "Per-link spatial covariance matrices of an antenna array, formed on the device: a dict of complex64 arrays "
          "(rx (num_rx, num_tx, 2, Nr, Nr), tx (num_rx, num_tx, 2, Nt, Nt), buffer); a side whose elements are None is "
          "not formed",
          py::arg("mesh_filepath"), py::arg("rx_positions"), py::arg("tx_positions"),
          py::arg("rx_velocities"), py::arg("tx_velocities"), py::arg("carrier_frequency"),
          py::arg("num_rx"), py::arg("num_tx"), py::arg("num_paths"), py::arg("num_bounces"),
          py::arg("rx_elements") = py::none(), py::arg("tx_elements") = py::none(), py::arg("los") = true,
          py::arg("scatter") = true, py::arg("array_frequency") = py::none(), py::arg("patterns") = py::none());
    m.def("compute_dominant_paths", &compute_dominant_paths_py,
          "The max_paths strongest paths of every link, selected on the device: a dict of arrays (kept, eligible, "
          "power, path, bounce, tri, a_te, a_tm, tau, freq_shift, u_rx, u_tx, buffer)",
          py::arg("mesh_filepath"), py::arg("rx_positions"), py::arg("tx_positions"),
          py::arg("rx_velocities"), py::arg("tx_velocities"), py::arg("carrier_frequency"),
          py::arg("num_rx"), py::arg("num_tx"), py::arg("num_paths"), py::arg("num_bounces"),
          py::arg("max_paths"), py::arg("los") = true, py::arg("scatter") = true,
          py::arg("patterns") = py::none());
    m.def("compute_sparse_array_channel", &compute_sparse_array_channel_py,
          "Antenna-array channel of the max_paths strongest paths of every link, selected and evaluated on the device: "
          "complex64 (num_rx, num_tx, Nr, Nt, 2, num_times, num_freqs); with return_paths=True the tuple (H, the lists as "
          "compute_dominant_paths returns them)",
          py::arg("mesh_filepath"), py::arg("rx_positions"), py::arg("tx_positions"),
          py::arg("rx_velocities"), py::arg("tx_velocities"), py::arg("carrier_frequency"),
          py::arg("num_rx"), py::arg("num_tx"), py::arg("num_paths"), py::arg("num_bounces"),
          py::arg("f0"), py::arg("df"), py::arg("num_freqs"), py::arg("rx_elements"), py::arg("tx_elements"),
          py::arg("max_paths"), py::arg("t0") = 0.0, py::arg("dt") = 0.0, py::arg("num_times") = 1,
          py::arg("los") = true, py::arg("scatter") = true, py::arg("array_frequency") = py::none(),
          py::arg("patterns") = py::none(), py::arg("return_paths") = false);
    m.def("compute_sparse_beam_channel", &compute_sparse_beam_channel_py,
          "Beamformed (codebook) channel of the max_paths strongest paths of every link, selected and evaluated on the "
          "device: complex64 (num_rx, num_tx, Br, Bt, 2, num_times, num_freqs); rx_weights (Br, Nr) is applied conjugated, "
          "tx_weights (Bt, Nt) as it is; with return_paths=True the tuple (B, the lists as compute_dominant_paths returns "
          "them)",
          py::arg("mesh_filepath"), py::arg("rx_positions"), py::arg("tx_positions"),
          py::arg("rx_velocities"), py::arg("tx_velocities"), py::arg("carrier_frequency"),
          py::arg("num_rx"), py::arg("num_tx"), py::arg("num_paths"), py::arg("num_bounces"),
          py::arg("f0"), py::arg("df"), py::arg("num_freqs"), py::arg("rx_elements"), py::arg("tx_elements"),
          py::arg("rx_weights"), py::arg("tx_weights"), py::arg("max_paths"), py::arg("t0") = 0.0, py::arg("dt") = 0.0,
          py::arg("num_times") = 1, py::arg("los") = true, py::arg("scatter") = true,
          py::arg("array_frequency") = py::none(), py::arg("patterns") = py::none(), py::arg("return_paths") = false);
    m.def("compute_sparse_array_taps", &compute_sparse_array_taps_py,
          "Antenna-array impulse responses of the max_paths strongest paths of every link, selected and evaluated on the "
          "device: complex64 (num_rx, num_tx, Nr, Nt, 2, num_times, num_taps); with return_paths=True the tuple (h, the "
          "lists as compute_dominant_paths returns them)",
          py::arg("mesh_filepath"), py::arg("rx_positions"), py::arg("tx_positions"),
          py::arg("rx_velocities"), py::arg("tx_velocities"), py::arg("carrier_frequency"),
          py::arg("num_rx"), py::arg("num_tx"), py::arg("num_paths"), py::arg("num_bounces"),
          py::arg("sampling_rate"), py::arg("num_taps"), py::arg("rx_elements"), py::arg("tx_elements"),
          py::arg("max_paths"), py::arg("l_min") = 0, py::arg("center_frequency") = py::none(), py::arg("t0") = 0.0,
          py::arg("dt") = 0.0, py::arg("num_times") = 1, py::arg("los") = true, py::arg("scatter") = true,
          py::arg("array_frequency") = py::none(), py::arg("patterns") = py::none(), py::arg("return_paths") = false);
    m.def("compute_sparse_beam_taps", &compute_sparse_beam_taps_py,
          "Beamformed (codebook) impulse responses of the max_paths strongest paths of every link, selected and evaluated "
          "on the device: complex64 (num_rx, num_tx, Br, Bt, 2, num_times, num_taps); rx_weights (Br, Nr) is applied "
          "conjugated, tx_weights (Bt, Nt) as it is; with return_paths=True the tuple (h, the lists as "
          "compute_dominant_paths returns them)",
          py::arg("mesh_filepath"), py::arg("rx_positions"), py::arg("tx_positions"),
          py::arg("rx_velocities"), py::arg("tx_velocities"), py::arg("carrier_frequency"),
          py::arg("num_rx"), py::arg("num_tx"), py::arg("num_paths"), py::arg("num_bounces"),
          py::arg("sampling_rate"), py::arg("num_taps"), py::arg("rx_elements"), py::arg("tx_elements"),
          py::arg("rx_weights"), py::arg("tx_weights"), py::arg("max_paths"), py::arg("l_min") = 0,
          py::arg("center_frequency") = py::none(), py::arg("t0") = 0.0, py::arg("dt") = 0.0, py::arg("num_times") = 1,
          py::arg("los") = true, py::arg("scatter") = true, py::arg("array_frequency") = py::none(),
          py::arg("patterns") = py::none(), py::arg("return_paths") = false);
    m.def("version", []() { return std::string(hrt_version()); });
    // Between calls the library keeps the device workspace and the page-locked staging of the last
    // call (C3: 3.3 GB of HBM, 0.4 GB of pinned host memory; up to HRT_POOL_MAX_BYTES, default 24 GiB)
    // and parked helper threads: this gives them back (csrc/host/compute_paths.c, hrt_cache_clear).
    m.def("cache_clear", []() { hrt_cache_clear(); },
          "Release the device / pinned buffers and helper threads kept between compute_paths calls");
}
