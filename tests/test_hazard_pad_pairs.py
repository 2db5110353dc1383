"""CPU: the hazard pass's register-pair rule (csrc/hazard_pad.py PAIR_STORE), applied to the translation units built
with the packed-FP32 forms: 64-bit VMEM stores and 64- / 128-bit LDS writes get the wait states of the wide stores."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "admm-deconv_amd", "csrc"))
import hazard_pad  # noqa: E402


def pad(*lines, pairs):
    text, n = hazard_pad.pad_asm("\n".join(lines), pairs)
    return text.split("\n"), n


def test_lds_pair_write_then_packed_write_is_padded_only_in_pair_mode():
    lines = ("\tds_write_b64 v176, v[68:69] offset:512", "\tv_pk_add_f32 v[68:69], v[60:61], v[62:63]")
    out, n = pad(*lines, pairs=True)
    assert n == 1 and out[1].strip() == "s_nop 1"
    out, n = pad(*lines, pairs=False)
    assert n == 0 and out == list(lines)


def test_second_data_operand_of_write2_and_64_bit_vmem_store():
    out, n = pad("\tds_write2_b64 v176, v[68:69], v[60:61] offset1:1", "\tv_pk_fma_f32 v[60:61], v[2:3], s[0:1], v[4:5]",
                 pairs=True)
    assert n == 1
    out, n = pad("\tbuffer_store_dwordx2 v[46:47], v189, s[24:27], s34 offen", "\tv_mov_b32_e32 v1, 0",
                 "\tv_pk_mul_f32 v[46:47], v[2:3], v[4:5]", pairs=True)
    assert n == 1 and out[2].strip() == "s_nop 0"   # one wait state already spent


def test_address_register_and_unrelated_writes_are_not_padded():
    out, n = pad("\tds_write_b64 v176, v[68:69]", "\tv_add_u32_e32 v176, 8, v176", "\tv_pk_add_f32 v[70:71], v[60:61], v[62:63]",
                 pairs=True)
    assert n == 0
