"""Channel code of the blind payload: the NumPy restatement of the rule as include/wmhip.h states it ("channel code") - the
rate-1/2 K = 7 encoder, the quantiser, the Viterbi forward pass with its decision words, the traceback - and the vectors and
cases the CPU and GPU tests share.  Written from the rule, not from payload.py: the product's encode_k7 / quantise_soft are
held against these.  Nothing here touches the device.

    encode    r = ((r << 1) | u_t) & 127 from r = 0 over u and 6 zeros; coded[2 t] = parity(r & 0o171), coded[2 t + 1] =
              parity(r & 0o133)
    quantise  L = int32(clip(rint(soft * (1024 / peak)), -1024, 1024)), peak = max |soft| or 1, float64
    forward   L clamped to +-1024; pm[0] = 0, pm[s != 0] = -2^30; new state s' from p_b = (s' >> 1) | (b << 5) with r_b = s' |
              (b << 6): c_b = pm[p_b] + (1 - 2 parity(r_b & 0o171)) L[2 t] + (1 - 2 parity(r_b & 0o133)) L[2 t + 1]; b = 1 iff
              c_1 > c_0; bit s' of D[t] = b
    back      s = 0 at the last step, down: u_t = s & 1, b = (D[t] >> s) & 1, s = (s >> 1) | (b << 5)
"""
import functools
import importlib

import numpy as np

import __graft_entry__ as ge
import payload_refs as pr
import payload_sync_refs as sr

P = importlib.import_module(ge.PKG_NAME + ".payload")
hg = importlib.import_module(ge.PKG_NAME + ".hostglue")

TAIL = 6
G0, G1 = 0o171, 0o133
LLR_MAX = 1024
PM_FLOOR = -(1 << 30)
MAX_STEPS = 1 << 18


def parity(x: int) -> int:
    return bin(int(x)).count("1") & 1


def encode_ref(u) -> np.ndarray:
    """the literal encoder: one register, one step at a time"""
    r, out = 0, []
    for b in [int(x) & 1 for x in np.asarray(u).reshape(-1)] + [0] * TAIL:
        r = ((r << 1) | b) & 127
        out += [parity(r & G0), parity(r & G1)]
    return np.array(out, np.uint8)


def quantise_ref(soft) -> np.ndarray:
    s = np.asarray(soft, np.float64)
    peak = float(np.abs(s).max()) if s.size else 0.0
    if peak == 0.0:
        peak = 1.0
    return np.clip(np.rint(s * (1024.0 / peak)), -1024, 1024).astype(np.int32)


_S = np.arange(64)
_SIGN0 = np.array([[1 - 2 * parity(s & g) for s in range(64)] for g in (G0, G1)], np.int64)        # the b = 0 branch (r_0 = s')
_SIGN1 = np.array([[1 - 2 * parity((s | 64) & g) for s in range(64)] for g in (G0, G1)], np.int64)  # the b = 1 branch
_P0, _P1 = _S >> 1, (_S >> 1) | 32


def viterbi_ref(L, n_info: int) -> tuple:
    """(info uint8 [n_info], final_metric int, decisions uint64 [n_info + 6]) of one codeword's int values L [2 (n_info + 6)];
    the 64 states of a step at once, both branch metrics from their own signs (bm_1 is not assumed to be -bm_0)"""
    n_steps = int(n_info) + TAIL
    L = np.clip(np.asarray(L, np.int64).reshape(-1), -LLR_MAX, LLR_MAX)
    assert L.size == 2 * n_steps and 1 <= n_info and n_steps <= MAX_STEPS
    pm = np.full(64, PM_FLOOR, np.int64)
    pm[0] = 0
    D = np.zeros(n_steps, np.uint64)
    weights = (np.uint64(1) << _S.astype(np.uint64))
    for t in range(n_steps):
        c0 = pm[_P0] + _SIGN0[0] * L[2 * t] + _SIGN0[1] * L[2 * t + 1]
        c1 = pm[_P1] + _SIGN1[0] * L[2 * t] + _SIGN1[1] * L[2 * t + 1]
        b = c1 > c0
        pm = np.where(b, c1, c0)
        D[t] = weights[b].sum(dtype=np.uint64)
    assert pm.min() > -(1 << 30) - (1 << 29) and pm.max() <= (1 << 29)      # the rule's range: int32 without normalising
    return traceback_ref(D, n_info), int(pm[0]), D


def traceback_ref(D, n_info: int) -> np.ndarray:
    s, u = 0, np.zeros(len(D), np.uint8)
    for t in range(len(D) - 1, -1, -1):
        u[t] = s & 1
        b = (int(D[t]) >> s) & 1
        s = (s >> 1) | (b << 5)
    return u[:n_info]


def viterbi_literal(L, n_info: int) -> tuple:
    """the same, one state at a time in Python integers, as the rule is written: what pins viterbi_ref's tie rule"""
    n_steps = n_info + TAIL
    L = [max(-LLR_MAX, min(LLR_MAX, int(x))) for x in np.asarray(L).reshape(-1)]
    pm = [0] + [PM_FLOOR] * 63
    D = []
    for t in range(n_steps):
        new, word = [0] * 64, 0
        for s in range(64):
            c = []
            for b in (0, 1):
                p, r = (s >> 1) | (b << 5), s | (b << 6)
                c.append(pm[p] + (1 - 2 * parity(r & G0)) * L[2 * t] + (1 - 2 * parity(r & G1)) * L[2 * t + 1])
            b = 1 if c[1] > c[0] else 0
            new[s] = c[b]
            word |= b << s
        pm = new
        D.append(word)
    return traceback_ref(D, n_info), pm[0], np.array(D, np.uint64)


# ---- the vectors the CPU tests, the host harness and the GPU tests share ------------------------------------------------
N_INFOS = (1, 57, 58, 59, 64, 121, 122, 123, 1000)      # n_steps 7, 63, 64, 65, 70, 127, 128, 129, 1006: the 64-step chunk edges
FLIP, ERASE = 0.08, 0.40


def _clean(n_info: int, seed: int):
    rng = np.random.default_rng([n_info, seed])
    u = rng.integers(0, 2, n_info).astype(np.uint8)
    c = encode_ref(u).astype(np.int64)
    # seeded magnitudes, as a quantised soft vector has them, the sign from the coded bit (positive: a 0)
    L = (1 - 2 * c) * rng.integers(200, 1025, c.size)
    return rng, u, L


def _flips(rng, size: int) -> np.ndarray:
    """8 % of the positions, spread: 2 seeded positions in every run of 25 values (a whole-sign flip at a seeded magnitude is a
    wrong vote at full weight; 8 % of them drawn independently bunch up past what any rate-1/2 code corrects at 1000 bits)"""
    flip = np.zeros(size, bool)
    for b0 in range(0, size, 25):
        m = min(25, size - b0)
        flip[b0 + rng.choice(m, 2 if m == 25 else int(round(m * FLIP)), replace=False)] = True
    return flip


# The seed of every noisy vector: the first of 1, 2, .. whose vector the restatement decodes (an erased run that covers all ten
# positions in which two paths differ leaves a tie, which the tie rule decides either way: about one vector in three at 1000
# bits).  test_payload_code asserts that each one decodes; the GPU tests compare bits with the restatement either way.
_NOISY_SEED = {("flip", 121): 2, ("erase", 121): 2, ("flip", 122): 2, ("flip", 1000): 3, ("erase", 1000): 3}


@functools.lru_cache(maxsize=None)
def vectors() -> tuple:
    """((name, n_info, u uint8 [n_info] or None, L int32 [2 (n_info + 6)]), ..): for every n_info of N_INFOS a noiseless vector,
    one with 8 % of the signs flipped and one with 40 % of the values set to 0 (u: what they must decode to); then the tie
    vectors (L = 0 throughout; L in {-1, 0, 1}), whose u is None - only the tie rule decides them."""
    out = []
    for n in N_INFOS:
        rng, u, L = _clean(n, 0)
        out.append((f"clean-{n}", n, u, L.astype(np.int32)))
        rng, u, L = _clean(n, _NOISY_SEED.get(("flip", n), 1))
        out.append((f"flip-{n}", n, u, np.where(_flips(rng, L.size), -L, L).astype(np.int32)))
        rng, u, L = _clean(n, _NOISY_SEED.get(("erase", n), 1))
        gone = rng.random(L.size) < ERASE
        out.append((f"erase-{n}", n, u, np.where(gone, 0, L).astype(np.int32)))
    for n in (6, 58, 123):
        out.append((f"zero-{n}", n, None, np.zeros(2 * (n + TAIL), np.int32)))
        out.append((f"unit-{n}", n, None, np.random.default_rng([n, 3]).integers(-1, 2, 2 * (n + TAIL)).astype(np.int32)))
    for v in out:
        v[3].setflags(write=False)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def decoded(name: str) -> tuple:
    """viterbi_ref of a named vector; computed once, shared"""
    _, n, _, L = next(v for v in vectors() if v[0] == name)
    r = viterbi_ref(L, n)
    r[0].setflags(write=False); r[2].setflags(write=False)
    return r


# ---- the cases of DESIGN.md section 14, "Channel code": what repetition alone loses -------------------------------------
DOCUMENT_DATA = (pr.DOCUMENT_PAYLOADS[1], bytes(range(20)))                 # 9 and 20 bytes on the 512-tile document host
CROP_CASE = dict(shape=(160, 256), seeds=(1, 3), data=bytes(range(12)), crop=(11, 21, 120, 200))


def document_key() -> bytes:
    return hg.derive_key("pw", pr.DOCUMENT_NONCE)


@functools.lru_cache(maxsize=None)
def document_decode(data: bytes, code: bool) -> dict:
    """The restatement's embed and decode of ``data`` on the document host (payload_refs.document_votes under the product's
    keyed map), without the code or with it: wrong = the frame bits that come back wrong, raw_wrong = the carried bits whose
    sign is wrong, sure = every carried bit's sign is beyond what the sigma bar could move."""
    H, W = pr.DOCUMENT
    Y = pr.document_host(H, W, pr.DOCUMENT_SEED)
    frame = P.payload_frame(data)
    carried = encode_ref(frame) if code else frame
    tbi, order, offs = P.payload_map(H // 8, W // 8, document_key(), carried.size)
    r = pr.document_votes(Y, carried, tbi, order, offs)
    got = viterbi_ref(quantise_ref(r["soft"]), frame.size)[0] if code else (r["soft"] < 0).astype(np.uint8)
    return dict(n_carried=int(carried.size), raw_wrong=int(np.count_nonzero(r["wrong"])), wrong=int(np.count_nonzero(got != frame)),
                unframed=P.payload_unframe(got), soft=r["soft"], sure=r["sure"])


def crop_map(code: bool, data: bytes = None) -> tuple:
    """(frame bits, carried bits, tile_bit_index [nby, nbx]) of the crop case (or of another payload on its host) under the
    keyed map of payload_sync_refs"""
    H, W = CROP_CASE["shape"]
    frame = P.payload_frame(CROP_CASE["data"] if data is None else data)
    carried = encode_ref(frame) if code else frame
    tbi = P.payload_map(H // 8, W // 8, sr.key(), carried.size)[0].reshape(H // 8, W // 8)
    return frame, carried, tbi


def read_located(r: dict, frame_bits: int, code: bool) -> tuple:
    """(data, valid, wrong-or-None) of a locate_ref result's soft values: their signs, or the restatement's decode"""
    got = viterbi_ref(quantise_ref(r["soft"]), frame_bits)[0] if code else (r["soft"] < 0).astype(np.uint8)
    return P.payload_unframe(got) + (got,)


@functools.lru_cache(maxsize=None)
def crop_table() -> np.ndarray:
    """uint16 [nby, nbx]: the dither table of the crop case (frame index 0)"""
    H, W = CROP_CASE["shape"]
    return P.dither_table(H // 8, W // 8, sr.key(), 0).reshape(H // 8, W // 8)


@functools.lru_cache(maxsize=None)
def crop_marked(seed: int, code: bool, dither: bool, bgr: bool, data: bytes = None) -> np.ndarray:
    """The restatement's stego plane of the crop case's host: Y marked directly, or (bgr) through the product's BGR path as
    payload_sync_refs.marked_bgr_y forms it - the plane the extract reads from what embed_payload_arrays returns."""
    import payload_dither_refs as pdr
    from oracle import wm_oracle as o
    H, W = CROP_CASE["shape"]
    _, carried, tbi = crop_map(code, data)

    def embed(Y):
        return (pdr.embed_ref(Y, carried[tbi], crop_table(), sr.DELTA) if dither else pr.embed_ref(Y, carried[tbi], sr.DELTA))["stego"]
    Y = pr.host(H, W, seed)
    if not bgr:
        st = embed(Y)
    else:
        ycc = o.bgr_to_ycrcb(np.repeat(Y[..., None], 3, -1)).copy()
        ycc[..., 0] = embed(ycc[..., 0])
        st = np.ascontiguousarray(o.bgr_to_ycrcb(o.ycrcb_to_bgr(ycc))[..., 0])
    st.setflags(write=False)
    return st


@functools.lru_cache(maxsize=None)
def crop_located(seed: int, code: bool, dither: bool, bgr: bool, crop: tuple = None, data: bytes = None) -> dict:
    """locate_ref (payload_sync_refs, or payload_keyed_sync_refs for the dithered twin) of the case's crop, with data / valid
    / got as read_located reads them"""
    import payload_keyed_sync_refs as kr
    frame, carried, tbi = crop_map(code, data)
    plane = sr.crop_of(crop_marked(seed, code, dither, bgr, data), crop or CROP_CASE["crop"])
    r = kr.locate_ref(plane, crop_table(), tbi, carried.size) if dither else sr.locate_ref(plane, tbi, carried.size)
    data, valid, got = read_located(r, frame.size, code)
    return dict(r, data=data, valid=bool(valid), got=got, erased=int(np.count_nonzero(r["count"] == 0)),
                wrong=int(np.count_nonzero(got != frame)))
