"""Host: the pair kernel's two forms in the cross-compiled assembly of k_fast2.hip (no GPU needed).

k_scl_fast2<R, IN, CRC> reads LLR rows: its channel read is the bare load, so the f64 instantiations hold no f64 division
(llr_from_y's 2 y / sigma / sigma is v_div_scale_f64 / v_rcp_f64 / v_div_fmas_f64 / v_div_fixup_f64 on gfx950).
k_scl_fast2_y<R, IN, CRC> converts y with sigma and does hold them.  Both forms exist for every <R, IN, CRC> the launcher
can pick, and the y form keeps the occupancy of the LLR form (the VGPR limit of three / four wavefronts per SIMD)."""
import os
import re
import shutil
import subprocess

import pytest

TYPES = [("dd", 168), ("ff", 128), ("fd", 128)]   # <R, IN> as mangled, VGPRs at 3 (f64) / 4 (f32) wavefronts per SIMD


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    import __graft_entry__ as g
    out = tmp_path_factory.mktemp("fast2") / "k_fast2.s"
    subprocess.check_call([hipcc] + g.HIPCC_FLAGS + ["-S", "--cuda-device-only", "-o", str(out), os.path.join(g.CSRC, "k_fast2.hip")],
                          cwd=g.CSRC, stderr=subprocess.DEVNULL)
    return out.read_text()


def _name(form, types, crc):
    base = "k_scl_fast2" + form
    return f"_ZN5polar{len(base)}{base}I{types}Lb{crc}EEEvNS_9SclParamsE"


def _body(txt, name):
    m = re.search(r"^" + re.escape(name) + r":", txt, re.M)
    assert m, name
    return txt[m.start():txt.index(".Lfunc_end", m.start())]


def test_both_forms_of_every_instantiation_are_kernels(asm):
    for types, max_vgpr in TYPES:
        for crc in (0, 1):
            for form in ("", "_y"):
                name = _name(form, types, crc)
                m = re.search(r"\.name:\s+" + re.escape(name) + r"\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n", asm)
                assert m, name
                assert int(m.group(1)) <= max_vgpr, (name, m.group(1))
                assert re.search(r"\.amdhsa_kernel\s+" + re.escape(name) + r"\n", asm), name


def test_llr_form_has_no_f64_division(asm):
    div = re.compile(r"^\s*(v_div_scale_f64|v_rcp_f64|v_div_fmas_f64|v_div_fixup_f64)\b", re.M)
    for crc in (0, 1):
        assert not div.findall(_body(asm, _name("", "dd", crc))), _name("", "dd", crc)
        # the y form is where the conversion lives: sigma is not folded away there
        assert len(div.findall(_body(asm, _name("_y", "dd", crc)))) >= 4, _name("_y", "dd", crc)
