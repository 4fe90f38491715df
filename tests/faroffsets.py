"""TEST INFRASTRUCTURE: spectra laid out so that element indices and byte offsets pass 2^31 and 2^32.

Every kernel finds its spectra through int64 peak offsets; `layout()` places real spectra where a 32-bit byte offset or a 32-bit
element index would wrap, without ever holding the arrays on the host.  The element order of a layout:

    near block   the real spectra, from element 0
    filler       F spectra of W = PYA_FAST_PEAKS points (the last one shorter), content a function of (index inside the
                 spectrum, number of the filler mod 4): ascending m/z on a fixed spacing, four intensity patterns
    straddler    one real spectrum with element `mark` inside it, at least 64 of its peaks on either side
    far block    the real spectra again: every element index at or above `mark`

The real spectra come as PSMs: 24 of cfg2, 12 of cfg4, one spectrum of more than PYA_FAST_PEAKS peaks (the general kernel), one
of a single peak, and a 25th cfg2 PSM that is the straddler.  Every filler spectrum carries the trivial PSM "SAK", n_of_mod 1.

The filler is made so that the transforms leave it alone under the parameters below (tests/test_faroffsets_host.py asserts it):
adjacent points are 0.23 apart -- no difference of two points is within DEISOTOPE's tol of an isotope spacing, every point is
isolated under CENTROID's gap, a precursor of charge 0 gives STRIP no window -- so the offsets behind a filler are known in
closed form: new_off == peak_off across it.

`fill(layout, device)` writes the filler on the device by assigning a tiled view of the uploaded patterns, chunk by chunk, and
copies the real spectra into place; `materialise(layout)` is the same thing in NumPy for the one mark that fits a host."""
import numpy as np

from pyascore_amd import _lib, rollup as ru, synth

W = 8192
MAX_PEAKS = 65535
assert W == getattr(_lib, "PYA_FAST_PEAKS", W)

HARNESS, M1, M2, M3 = 2 ** 16, 2 ** 29, 2 ** 31, 2 ** 32
#: name -> (mark, m/z dtype, intensity dtype).  HARNESS proves the builder where everything is also checked on the CPU; M1: byte
#: offset 2^32 in float64; M2: an int32 element index wraps (byte offset 2^33); M3: a uint32 element index wraps
MARKS = {"HARNESS": (HARNESS, np.float64, np.float64), "M1": (M1, np.float64, np.float64),
         "M2": (M2, np.float32, np.float32), "M3": (M3, np.float32, np.float32)}
SEED = 20261
CAP_BYTES = 40 * 10 ** 9            # the device bytes one GPU test may need

N_CFG2, N_CFG4 = 24, 12
N_NEAR = N_CFG2 + N_CFG4 + 2        # ... + the big spectrum + the one-peak spectrum
BIG_PEAKS = 9000
SETTINGS = {"cfg2": synth.describe("cfg2", 1)["settings"],          # plain, fast routes
            "cfg4": synth.describe("cfg4", 1)["settings"]}          # charges, neutral loss, b/y/c/z: the general front end

SPACING, MZ0 = 0.23, 100.0
_IT_MOD, _IT_MUL = 8209, (3571, 2477, 5003, 6007)                   # (8209 is prime: i -> i * mul mod 8209 has no repeat below it)

DEISOTOPE = ru.deisotope_params(tol=0.02, max_charge=3)
DECHARGE = ru.decharge_params(tol=0.02, max_charge=3)
STRIP = ru.strip_params(tol=1.5, losses=(97.976896,))
CENTROID = ru.centroid_params(gap=0.2, half_width=4)
MARKERS = ru.marker_params(mz=(126.1277, 216.0426, 500.25), losses=(97.976896,), tol=0.5)
CAL_KNOTS = [32.0, 28.0, 22.0, 15.0, 9.0, 4.0, 0.0, -3.0]


def filler_patterns(mz_dtype, it_dtype):
    """``(mz[W], intensity[4, W])`` of the filler: the m/z ascend by SPACING from MZ0, the four intensity rows are
    permutations of distinct positive integers (no ties: the common binning kernel takes them)."""
    i = np.arange(W, dtype=np.int64)
    mz = (MZ0 + SPACING * i.astype(np.float64)).astype(mz_dtype)
    it = np.stack([100 + (i * m) % _IT_MOD for m in _IT_MUL]).astype(it_dtype)
    assert all(np.unique(row).size == W for row in it) and (np.diff(mz.astype(np.float64)) > 0.2).all()
    return mz, it


def filler_spectrum(mz_dtype, it_dtype, j, length=W):
    """filler number ``j`` (counted from the first filler) cut to ``length`` points"""
    mz, it = filler_patterns(mz_dtype, it_dtype)
    return mz[:length].copy(), it[j % 4][:length].copy()


def _real_psms(seed):
    """the 39 real PSMs in float64: near block order, the straddler last"""
    def psms_of(batch):
        return [dict(mz=kw["mz_arr"], intensity=kw["int_arr"], peptide=kw["peptide"], n_of_mod=kw["n_of_mod"],
                     max_charge=kw["max_fragment_charge"]) for kw in (synth.unpack_psm(batch, i) for i in range(batch["n_psm"]))]
    cfg2 = psms_of(synth.make_batch("cfg2", n_psm=N_CFG2 + 1, seed=seed)[0])
    cfg4 = psms_of(synth.make_batch("cfg4", n_psm=N_CFG4, seed=seed + 1)[0])
    rng = np.random.default_rng([seed, 0xFA2])
    big = dict(mz=np.sort(rng.uniform(100.0, 3000.0, BIG_PEAKS)), intensity=rng.lognormal(5.0, 1.0, BIG_PEAKS),
               peptide="ASTLGYKRSTYAGK", n_of_mod=2, max_charge=2)
    one = dict(mz=np.array([650.3]), intensity=np.array([321.0]), peptide="ASTLGYKRSTYAGK", n_of_mod=2, max_charge=2)
    return cfg2[:N_CFG2] + cfg4 + [big, one, cfg2[N_CFG2]]


class Layout:
    """Offsets of a layout and the host copies of its real spectra (``real``: a CSR batch from offset 0 of the 39 real PSMs in
    the layout's dtypes, the straddler last).  Spectrum numbers: ``near`` / ``filler`` / ``straddler`` / ``far`` (ranges and one
    number); ``real_of[s]`` is the PSM of ``real`` that spectrum s is a copy of, -1 for a filler."""

    def __init__(self, name, mark, mz_dtype, it_dtype, seed):
        self.name, self.mark, self.seed = name, int(mark), seed
        self.mz_dtype, self.it_dtype = np.dtype(mz_dtype), np.dtype(it_dtype)
        self.real = synth.narrow_batch(synth.pack_batch(_real_psms(seed)), mz_dtype, it_dtype)
        sizes = np.diff(self.real["peak_off"])
        near_end = int(sizes[:N_NEAR].sum())
        s_len = int(sizes[N_NEAR])
        before = s_len // 2 + (1 if (s_len // 2) % 64 == 0 else 0)   # the mark in the middle of the straddler, inside a stride
        s_start = self.mark - before
        gap = s_start - near_end
        if gap < W:
            raise ValueError("mark %d leaves no room for a filler behind the near block" % mark)
        self.n_filler = -(-gap // W)
        self.last_len = gap - (self.n_filler - 1) * W                 # 1 .. W
        counts = np.concatenate([sizes[:N_NEAR], np.full(self.n_filler - 1, W), [self.last_len, s_len], sizes[:N_NEAR]])
        self.peak_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        self.n_spectra = counts.size
        self.near = range(0, N_NEAR)
        self.filler = range(N_NEAR, N_NEAR + self.n_filler)
        self.straddler = N_NEAR + self.n_filler
        self.far = range(self.straddler + 1, self.n_spectra)
        self.real_of = np.full(self.n_spectra, -1, np.int64)
        self.real_of[:N_NEAR] = np.arange(N_NEAR)
        self.real_of[self.straddler] = N_NEAR
        self.real_of[self.straddler + 1:] = np.arange(N_NEAR)
        self.filler_begin, self.filler_end = int(self.peak_off[N_NEAR]), int(self.peak_off[self.straddler])
        self.total = int(self.peak_off[-1])

    # ---- the PSMs ----
    def real_spectra(self):
        """the spectrum numbers that hold real spectra: near block, straddler, far block"""
        return np.flatnonzero(self.real_of >= 0)

    def batch(self):
        """The CSR batch of the whole layout WITHOUT spectrum arrays (a ``DevicePlan`` reads none): one PSM per spectrum, the
        real ones with their peptides, every filler with "SAK"."""
        r = self.real
        peps, k, z = [], np.ones(self.n_spectra, np.int32), np.ones(self.n_spectra, np.int32)
        lens = np.full(self.n_spectra, 3, np.int64)
        for s in self.real_spectra():
            i = int(self.real_of[s])
            lens[s] = r["pep_off"][i + 1] - r["pep_off"][i]
            k[s], z[s] = r["n_of_mod"][i], r["max_charge"][i]
        pep_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        pep = np.zeros(int(pep_off[-1]), np.uint8)
        f0, f1 = int(pep_off[self.filler[0]]), int(pep_off[self.straddler])
        pep[f0:f1] = np.tile(np.frombuffer(b"SAK", np.uint8), self.n_filler)
        for s in self.real_spectra():
            i = int(self.real_of[s])
            pep[pep_off[s]:pep_off[s + 1]] = r["pep"][r["pep_off"][i]:r["pep_off"][i + 1]]
        return dict(n_psm=self.n_spectra, peak_off=self.peak_off, pep=pep, pep_off=pep_off, n_of_mod=k, max_charge=z,
                    aux_pos=np.zeros(0, np.uint32), aux_mass=np.zeros(0, np.float32), aux_off=np.zeros(self.n_spectra + 1, np.int64))

    def alone(self, spectra):
        """the real PSMs behind the spectrum numbers ``spectra`` as a batch of their own from offset 0, in that order"""
        r = self.real
        psms = []
        for s in spectra:
            kw = synth.unpack_psm(r, int(self.real_of[s]))
            psms.append(dict(mz=kw["mz_arr"], intensity=kw["int_arr"], peptide=kw["peptide"], n_of_mod=kw["n_of_mod"],
                             max_charge=kw["max_fragment_charge"]))
        return synth.pack_batch(psms)

    def filler_alone(self):
        """the four filler patterns and the short last filler (number 4) with "SAK" as a batch from offset 0"""
        last = self.n_filler - 1
        psms = [dict(zip(("mz", "intensity"), filler_spectrum(self.mz_dtype, self.it_dtype, j)), peptide="SAK", n_of_mod=1, max_charge=1)
                for j in range(4)]
        psms.append(dict(zip(("mz", "intensity"), filler_spectrum(self.mz_dtype, self.it_dtype, last, self.last_len)),
                         peptide="SAK", n_of_mod=1, max_charge=1))
        return synth.pack_batch(psms)

    def precursors(self, spectra=None):
        """``(prec_mz float64, prec_z int32)`` per spectrum: a real spectrum has charge 2 and the m/z of its middle peak (STRIP
        cuts around it), a filler charge 0 -- unusable, no window"""
        spectra = np.arange(self.n_spectra) if spectra is None else np.asarray(spectra)
        pm, pz = np.zeros(spectra.size, np.float64), np.zeros(spectra.size, np.int32)
        r = self.real
        for at, s in enumerate(spectra):
            i = int(self.real_of[s])
            if i >= 0:
                a, b = int(r["peak_off"][i]), int(r["peak_off"][i + 1])
                pm[at], pz[at] = float(r["mz"][(a + b) // 2]), 2
        return pm, pz

    # ---- device bytes ----
    def array_bytes(self):
        """the two spectrum arrays of the whole layout"""
        return self.total * (self.mz_dtype.itemsize + self.it_dtype.itemsize)

    def keep_bytes(self, n_spectra=None):
        """an upper bound of the workspace of strip / deisotope / centroid over spectra that end at ``total``: the keep words,
        one more per spectrum, the tile sums of the scan (at most one per spectrum)"""
        n = self.n_spectra if n_spectra is None else n_spectra
        return 8 * ((self.total >> 6) + 2 * n + 2)

    def plan_bytes(self):
        """What a plan over the whole layout holds at least: an 8-byte retained entry for every raw peak (each spectrum's count
        rounded up to even), the 256-cell m/z grid and some hundred bytes of offsets, descriptors and lists per PSM.  The
        tests assert the exact ``pya_plan_workspace_bytes`` against the cap once the plan exists."""
        sizes = np.diff(self.peak_off)
        return 8 * int(((sizes + 1) & ~1).sum()) + self.n_spectra * (512 + 256)

    def device_bytes(self, test):
        """What a GPU test of tests/test_gpu_far_offsets.py has resident at its peak: ``plan`` / ``stages`` the two arrays, the
        plan (``plan_bytes``) and the result rows, ``far_input`` the arrays, the keep words and outputs of the size of the real
        spectra, ``recalibrate`` the arrays and a second m/z array, ``recalibrate_in_place`` the arrays alone, ``far_output`` the
        arrays twice and the keep words."""
        arrays, n = self.array_bytes(), self.n_spectra
        real_bytes = int(self.real["peak_off"][-1]) * 2 * 16
        if test == "plan":
            return arrays + self.plan_bytes() + n * (4 + 8 + 4 + 3 * (4 + 8))
        if test == "stages":
            return arrays + self.plan_bytes() + n * (4 + 8 + 4 + 3 * (4 + 8) + 64 + 3 * 16 + 16 + 8 * 16 + 8 + 8) + 64 * 16 * n
        if test == "far_input":
            return arrays + self.keep_bytes(N_NEAR + 1) + real_bytes
        if test == "recalibrate":
            return arrays + self.total * self.mz_dtype.itemsize
        if test == "recalibrate_in_place":
            return arrays + real_bytes
        if test == "far_output":
            return 2 * arrays + self.keep_bytes() + 16 * n
        raise KeyError(test)


_layouts = {}


def layout(mark, mz_dtype=None, it_dtype=None, seed=SEED):
    """The layout of a mark: by name (``"M2"``) or as ``(mark, mz_dtype, it_dtype)``.  Made once per process and shared."""
    if isinstance(mark, str):
        name = mark
        mark, mz_dtype, it_dtype = MARKS[name]
    else:
        name = "mark_%d" % mark
    key = (int(mark), np.dtype(mz_dtype).name, np.dtype(it_dtype).name, seed)
    if key not in _layouts:
        _layouts[key] = Layout(name, mark, mz_dtype, it_dtype, seed)
    return _layouts[key]


def materialise(lay):
    """``(mz, intensity)`` of the whole layout as NumPy arrays (only where that is small: the HARNESS mark)"""
    if lay.total > 1 << 24:
        raise ValueError("materialise is for the harness mark; the large ones are filled on the device")
    mz, it = np.empty(lay.total, lay.mz_dtype), np.empty(lay.total, lay.it_dtype)
    pat_mz, pat_it = filler_patterns(lay.mz_dtype, lay.it_dtype)
    for j, s in enumerate(lay.filler):
        a, b = int(lay.peak_off[s]), int(lay.peak_off[s + 1])
        mz[a:b], it[a:b] = pat_mz[:b - a], pat_it[j % 4][:b - a]
    r = lay.real
    for s in lay.real_spectra():
        i = int(lay.real_of[s])
        a, b = int(r["peak_off"][i]), int(r["peak_off"][i + 1])
        mz[lay.peak_off[s]:lay.peak_off[s + 1]], it[lay.peak_off[s]:lay.peak_off[s + 1]] = r["mz"][a:b], r["intensity"][a:b]
    return mz, it


def fill(lay, device, chunk=2048):
    """``(d_mz, d_intensity)``: the whole layout as two device tensors.  The filler is written ``chunk`` spectra at a time by
    assigning the four uploaded patterns to a ``[groups, 4, W]`` view; the real spectra are copied into place; the host never
    holds more than the patterns and the real spectra."""
    import torch
    pat_mz, pat_it = filler_patterns(lay.mz_dtype, lay.it_dtype)
    d_pat_mz, d_pat_it = torch.from_numpy(pat_mz).to(device), torch.from_numpy(pat_it).to(device)
    d_mz = torch.empty(lay.total, dtype=d_pat_mz.dtype, device=device)
    d_it = torch.empty(lay.total, dtype=d_pat_it.dtype, device=device)
    full = lay.n_filler - 1
    chunk -= chunk % 4
    for j0 in range(0, full, chunk):
        j1 = min(full, j0 + chunk)
        a = lay.filler_begin + j0 * W
        groups, rest = divmod(j1 - j0, 4)
        if groups:
            d_mz[a:a + groups * 4 * W].view(groups * 4, W)[:] = d_pat_mz
            d_it[a:a + groups * 4 * W].view(groups, 4, W)[:] = d_pat_it
        for j in range(j1 - rest, j1):                                # (j0 is a multiple of 4: filler j has pattern j % 4)
            b = lay.filler_begin + j * W
            d_mz[b:b + W] = d_pat_mz
            d_it[b:b + W] = d_pat_it[j % 4]
    a = lay.filler_begin + full * W
    d_mz[a:a + lay.last_len] = d_pat_mz[:lay.last_len]
    d_it[a:a + lay.last_len] = d_pat_it[full % 4][:lay.last_len]
    r = lay.real
    d_real_mz, d_real_it = torch.from_numpy(r["mz"]).to(device), torch.from_numpy(r["intensity"]).to(device)
    for s in lay.real_spectra():
        i = int(lay.real_of[s])
        a, b = int(r["peak_off"][i]), int(r["peak_off"][i + 1])
        d_mz[int(lay.peak_off[s]):int(lay.peak_off[s + 1])] = d_real_mz[a:b]
        d_it[int(lay.peak_off[s]):int(lay.peak_off[s + 1])] = d_real_it[a:b]
    return d_mz, d_it
