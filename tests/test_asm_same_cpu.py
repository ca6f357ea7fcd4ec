"""tools/asm_same.py on three tiny hand-written two-kernel texts: one result of each class, and the exit status."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("asm_same", os.path.join(ROOT, "tools", "asm_same.py"))
asm_same = importlib.util.module_from_spec(spec)
spec.loader.exec_module(asm_same)


def kernel(name, body, vgpr=12, first_label=0):
    """One kernel as the compiler writes it: its text, then its descriptor."""
    body = body.replace("L0", f".LBB{first_label}_1").replace("L1", f".LBB{first_label}_2")
    return f"""\t.globl\t{name}
\t.type\t{name},@function
{name}:                                 ; @{name}
; %bb.0:
{body}
\ts_endpgm
.Lfunc_end{first_label}:
\t.size\t{name}, .Lfunc_end{first_label}-{name}
\t.section\t.rodata,"a",@progbits
\t.amdhsa_kernel {name}
\t\t.amdhsa_next_free_vgpr {vgpr}
\t\t.amdhsa_next_free_sgpr 16
\t\t.amdhsa_private_segment_fixed_size 0
\t.end_amdhsa_kernel
\t.text
"""


BODY_A = """\ts_load_dwordx2 s[0:1], s[4:5], 0x0
\tv_mov_b32_e32 v1, 0            ; a comment
\ts_mov_b32 s2, 1
\ts_mov_b32 s3, 2
\ts_cbranch_scc1 L0
\tv_add_u32_e32 v1, v1, v0
L0:                                ; %bb.2
\ts_cbranch_execz L1
\tglobal_store_dword v0, v1, s[0:1]
L1:
\ts_nop 0"""
BODY_B = """\tv_mov_b32_e32 v2, 7
\tglobal_store_dword v0, v2, s[0:1]"""
SWAPPED = BODY_A.replace("\ts_mov_b32 s2, 1\n\ts_mov_b32 s3, 2", "\ts_mov_b32 s3, 2\n\ts_mov_b32 s2, 1")
ADDED = BODY_B + "\n\ts_nop 1"


def unit(a=BODY_A, b=BODY_B, cuid="1234", first_label=0, vgpr_b=12):
    return (kernel("k_one", a, first_label=first_label) + kernel("k_two", b, vgpr=vgpr_b, first_label=first_label + 1) +
            f"\t.type\t__hip_cuid_{cuid},@object\n\t.globl\t__hip_cuid_{cuid}\n__hip_cuid_{cuid}:\n\t.byte\t0\n")


def test_identical_but_for_labels_comments_and_cuid():
    tree = unit(cuid="abcd", first_label=5).replace("; a comment", "; another").replace(
        "\ts_mov_b32 s2, 1", "\t.loc\t1 20 3\n\ts_mov_b32 s2, 1")
    assert asm_same.compare_texts(unit(), tree) == {"k_one": "identical", "k_two": "identical"}


def test_two_adjacent_lines_swapped_is_reordered():
    assert asm_same.compare_texts(unit(), unit(a=SWAPPED)) == {"k_one": "reordered", "k_two": "identical"}


def test_descriptor_line_or_added_instruction_is_changed():
    assert asm_same.compare_texts(unit(), unit(vgpr_b=13)) == {"k_one": "identical", "k_two": "changed"}
    assert asm_same.compare_texts(unit(), unit(b=ADDED)) == {"k_one": "identical", "k_two": "changed"}
    # a swap with another register count is no reordering, and neither is a kernel only one side has
    assert asm_same.compare_texts(unit(), unit(a=SWAPPED).replace("next_free_sgpr 16", "next_free_sgpr 18"))["k_one"] == "changed"
    assert asm_same.compare_texts(unit(), kernel("k_one", BODY_A)) == {"k_one": "identical", "k_two": "changed"}


def test_exit_status_and_report(tmp_path, capsys):
    for name, text in (("parent", unit()), ("same", unit(cuid="ef01", first_label=3)), ("swapped", unit(a=SWAPPED)), ("more", unit(b=ADDED))):
        os.makedirs(tmp_path / name)
        (tmp_path / name / "render_x.s").write_text(text)
    parent = str(tmp_path / "parent")
    assert asm_same.main([parent, str(tmp_path / "same")]) == 0
    assert "render_x.s: 2 identical, 0 reordered, 0 changed" in capsys.readouterr().out
    assert asm_same.main([parent, str(tmp_path / "swapped")]) == 0
    out = capsys.readouterr().out
    assert "render_x.s: 1 identical, 1 reordered, 0 changed" in out and "reordered: k_one" in out
    assert asm_same.main([parent, str(tmp_path / "more")]) == 1
    assert "changed: k_two" in capsys.readouterr().out
