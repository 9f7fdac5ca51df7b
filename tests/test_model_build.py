"""tests/model_build.py itself: a program compiles and runs with and without the sanitizers and its exit status comes through,
a failed compile raises with the compiler's message, and a shared library cannot be asked for sanitizers."""
import subprocess

import pytest

import model_build

SANITIZE = ("-fsanitize=address,undefined", "-fno-sanitize-recover=all")


def source(tmp_path, text):
    path = tmp_path / "three_lines.cpp"
    path.write_text(text)
    return path


@pytest.mark.parametrize("sanitize", [(), SANITIZE], ids=["plain", "sanitized"])
def test_a_program_runs_and_its_exit_status_is_reported(tmp_path, sanitize):
    if sanitize:
        model_build.sanitizer_runtimes_or_skip()
    src = source(tmp_path, "#include <cstdlib>\nint main(int argc, char** argv) {\n    return argc > 1 ? std::atoi(argv[1]) : 0; }\n")
    exe = model_build.program([src], tmp_path, "three_lines", sanitize=sanitize)
    assert subprocess.run([exe]).returncode == 0
    assert subprocess.run([exe, "3"]).returncode == 3  # (a deliberately failing main)


def test_a_syntax_error_raises_with_the_compilers_message(tmp_path):
    src = source(tmp_path, "int main() {\n    return 0 +;\n}\n")
    with pytest.raises(AssertionError, match=r"three_lines\.cpp:2:\d+: error: expected primary-expression"):
        model_build.program([src], tmp_path, "never")
    with pytest.raises(AssertionError, match="expected primary-expression"):
        model_build.library([src], tmp_path, "libnever.so")


def test_a_library_takes_no_sanitizers(tmp_path):
    src = source(tmp_path, 'extern "C" int three() { return 3; }\n')
    with pytest.raises(TypeError):
        model_build.library([src], tmp_path, "libthree.so", sanitize=SANITIZE)
