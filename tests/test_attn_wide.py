"""icd_attention_wide (flash attention at head dims 168 ... 512, csrc/attention_wide.hip) on the host: what the entry refuses before a
launch, what icd_attention_plan reports for it (entry kind 3: family 4, NW = ceil(d / 128) waves per block, a block per 32-query tile of
each (sample, head), two LDS exchange buffers of NW x 8 KiB), and the rule by which AutoencoderKL reaches it.  No GPU."""
import ctypes as C

import pytest

from invertible_cd_amd import _lib

P0 = 1 << 20                                        # a 16-byte aligned non-null pointer (never dereferenced: every case is refused or planned)
WIDE = 3                                            # icd_attention_query.entry


def _wide(**kw):
    """icd_attention_wide on B = 2, H = 2, Nq = Nk = 35 with minimal leading dims, `kw` overriding -> status"""
    a = dict(q=P0, k=P0, vt=P0, out=P0, B=2, H=2, Nq=35, Nk=35, d=256, vt_bs=0, scale=0.0625)
    a.update({k: v for k, v in kw.items() if not k.startswith("ld")})
    hd = a["H"] * a["d"]
    a.update(dict(dict(ldq=hd, ldk=hd, ldvt=40, ldo=hd), **{k: v for k, v in kw.items() if k.startswith("ld")}))
    return _lib.load().icd_attention_wide(a["q"], a["k"], a["vt"], a["out"], a["B"], a["H"], a["Nq"], a["Nk"], a["d"], a["ldq"], a["ldk"],
                                          a["ldvt"], a["ldo"], a["vt_bs"], a["scale"], None)


def _plan(B, H, Nq, Nk, d):
    query, info = _lib.AttentionQuery(WIDE, B, H, Nq, Nk, d, 0, 0, 0, 0), _lib.AttentionInfo()
    return _lib.load().icd_attention_plan(C.byref(query), C.byref(info)), info


@pytest.mark.parametrize("d", [160, 164, 520, 0])
def test_head_dims_outside_168_to_512_are_refused_with_the_range_in_the_message(d):
    assert _wide(d=d) == -2                                                 # ICD_ERR_UNSUPPORTED, as icd_attention_masked's head dims
    msg = _lib.load().icd_last_error()
    assert b"icd_attention_wide" in msg and b"168 ... 512" in msg and str(d).encode() in msg, msg
    assert _plan(2, 2, 35, 35, d)[0] == -2 and b"168 ... 512" in _lib.load().icd_last_error()


REFUSALS = [
    ("null q", dict(q=None), "null pointer"), ("null k", dict(k=None), "null pointer"), ("null vt", dict(vt=None), "null pointer"),
    ("null out", dict(out=None), "null pointer"),
    ("ldq < H d", dict(ldq=504), "H * d"), ("ldk < H d", dict(ldk=504), "H * d"), ("ldo < H d", dict(ldo=508), "H * d"),
    ("ldq % 8", dict(ldq=516), "16-byte aligned"), ("ldvt % 8", dict(ldvt=44), "16-byte aligned"), ("ldvt < Nk", dict(ldvt=32), "ldvt >= Nk"),
    ("ldo % 4", dict(ldo=514), "16-byte aligned"), ("q alignment", dict(q=P0 + 8), "16-byte aligned"), ("out alignment", dict(out=P0 + 4), "8-byte"),
    ("vt_bs", dict(vt_bs=512 * 40 - 8), "vt_batch_stride"), ("Nk = 0", dict(Nk=0), "empty shape"), ("scale", dict(scale=0.0), "scale"),
    ("grid", dict(B=1 << 15, H=1 << 10, ldq=1 << 18, ldk=1 << 18, ldo=1 << 18), "grid limit"),
]


@pytest.mark.parametrize("name,kw,fragment", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_the_entry_refuses_before_any_launch(name, kw, fragment):
    assert _wide(**kw) == -1, name                                          # ICD_ERR_INVALID_ARG
    msg = _lib.load().icd_last_error()
    assert b"icd_attention_wide" in msg and fragment.encode() in msg, (name, msg)


@pytest.mark.parametrize("d", [168, 512])
def test_the_ends_of_the_range_pass_validation(d):
    assert _plan(2, 2, 35, 35, d)[0] == 0, _lib.load().icd_last_error()


@pytest.mark.parametrize("d,nw", [(168, 2), (256, 2), (264, 3), (384, 3), (392, 4), (512, 4)])
def test_the_plan_reports_waves_grid_and_lds(d, nw):
    for B, H, Nq, Nk in ((2, 2, 35, 35), (1, 1, 1, 1), (3, 1, 4096, 4096), (1, 1, 16384, 16384), (2, 3, 33, 129)):
        rc, p = _plan(B, H, Nq, Nk, d)
        assert rc == 0, _lib.load().icd_last_error()
        assert (p.family, p.variants, p.variant, p.NW) == (4, 3, nw - 2, nw) and nw == -(-d // 128)
        assert p.grid_x * p.grid_y * p.grid_z == -(-Nq // 32) * B * H and min(p.grid_x, p.grid_y, p.grid_z) >= 1
        assert p.lds_bytes == 2 * nw * 8192 and p.lds_bytes <= 160 * 1024
        assert (p.KS, p.DT, p.NT) == (8, 4, 2)                               # per wave: a 128-column slice, 64 keys per step
        assert (p.QT, p.OCC, p.NST, p.MODE, p.DR, p.causal, p.STL, p.tiles_per_wave, p.SPLIT, p.EPI, p.FEW) == (0,) * 11


def test_the_other_entry_kinds_keep_their_numbers():
    """the new kind is appended: 0 fused, 1 probs, 2 masked answer as before, 4 does not exist"""
    lib = _lib.load()
    for entry, family in ((0, 0), (1, 2), (2, 3)):
        query, info = _lib.AttentionQuery(entry, 2, 2, 35, 35, 64, 40, 0, 0, 0), _lib.AttentionInfo()
        assert lib.icd_attention_plan(C.byref(query), C.byref(info)) == 0 and info.family == family and info.NW == 0
    query = _lib.AttentionQuery(4, 2, 2, 35, 35, 256, 40, 0, 0, 0)
    assert lib.icd_attention_plan(C.byref(query), C.byref(_lib.AttentionInfo())) == -1 and b"entry" in lib.icd_last_error()


def test_the_vae_reaches_the_wide_kernel_by_the_documented_rule():
    """AutoencoderKL._attention_kind (a pure function of the switch and the shape): True takes a flash kernel wherever one has the head
    dim, False never, the default takes the wide kernel where one sample's scores exceed the 1 GiB step of the materialised path (it was
    measured slower below that: profiles/attn_wide.txt)."""
    from types import SimpleNamespace
    from invertible_cd_amd import vae
    kind = vae.AutoencoderKL._attention_kind

    def k(switch, B, N, Cc):
        return kind(SimpleNamespace(fused_attention=switch), B, N, Cc, (N + 7) // 8 * 8)
    assert [k(True, 2, 48, c) for c in (128, 160, 192, 512, 544)] == ["fused", "fused", "wide", "wide", "scores"]
    assert [k(False, 2, 48, c) for c in (128, 192, 512, 544)] == ["scores"] * 4
    assert k(None, 2, 48, 128) == "fused" and k(None, 2, 48, 544) == "scores" and k(None, 1, 32768, 544) == "scores"
    assert k(None, 1, 16392, 512) == "wide" and k(None, 8, 32768, 192) == "wide"      # more than 1 GiB of scores for one sample
    assert k(None, 8, 16384, 512) == "scores" and k(None, 8, 4096, 512) == "scores" and k(None, 2, 48, 192) == "scores"
