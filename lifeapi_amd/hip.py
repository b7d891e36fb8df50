"""ctypes binding of the C ABI in include/lifeapi_hip.h.

Import order matters: torch is imported first so that its bundled HIP runtime
(SONAME ``libamdhip64.so.7``) is the one ``liblifeapi_hip.so`` binds to --
device pointers and streams handed over from torch then belong to the same
runtime.  There is no fallback of any kind: a missing or unloadable library
raises ImportError, and every failed call raises :class:`LifeApiError`.

Universes are int64 tensors of shape (n, 64) holding the reference's
``LifeState::state`` words bit-for-bit (LifeAPI.hpp:39-40).
"""
from __future__ import annotations

import ctypes
import os

import numpy as np
import torch  # noqa: F401  (must precede loading the HIP library)

from .layout import N

# (LIFEAPI_HIP_LIB: another build of the same library, for A/B probes under tools/)
LIB_PATH = os.environ.get("LIFEAPI_HIP_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                                             "liblifeapi_hip.so")

if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} is missing: build it with "
        "`python -c 'import __graft_entry__ as g; g.build()'` (hipcc --offload-arch=gfx950)")
lib = ctypes.CDLL(LIB_PATH)

class LifeApiError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"lifeapi error {code}: {msg}")
        self.code = code


_vp, _sz, _u32, _u64, _int = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int
_SIGS = {
    "lifeapi_abi_version": ([], _int),
    "lifeapi_last_error": ([], ctypes.c_char_p),
    "lifeapi_device_count": ([], _int),
    "lifeapi_step_kernel_name": ([_u32], ctypes.c_char_p),
    "lifeapi_step_kernel_name_n": ([_u32, _sz], ctypes.c_char_p),
    "lifeapi_step_batch_dev": ([_vp, _vp, _sz, _u32, _vp], _int),
    "lifeapi_pop_batch_dev": ([_vp, _vp, _sz, _vp], _int),
    "lifeapi_hash_batch_dev": ([_vp, _vp, _sz, _vp], _int),
    "lifeapi_contains_batch_dev": ([_vp, _vp, _vp, _vp, _sz, _vp], _int),
    "lifeapi_step_contains_batch_dev": ([_vp, _vp, _vp, _vp, _vp, _sz, _u32, _vp], _int),
    "lifeapi_fill_random_dev": ([_vp, _sz, _u64, _u64, _int, _vp], _int),
    "lifeapi_weld_step_batch_dev": ([_vp, _sz, _u32, _vp], _int),
    "lifeapi_stable_pass_batch_dev": ([_vp, _vp, _sz, _int, _u32, _vp], _int),
    "lifeapi_neighbour_count_batch_dev": ([_vp, _vp, _sz, _vp], _int),
    "lifeapi_interaction_counts_batch_dev": ([_vp, _vp, _sz, _int, _vp], _int),
    "lifeapi_refined_step_batch_dev": ([_vp, _vp, _sz, _vp], _int),
    "lifeapi_step_batch": ([_vp, _vp, _sz, _u32, _int], _int),
    "lifeapi_host_register": ([_vp, _sz], _int),
    "lifeapi_step_contains_batch": ([_vp, _vp, _vp, _vp, _vp, _sz, _u32, _int], _int),
    "lifeapi_host_unregister": ([_vp], _int),
    "lifeapi_pop_batch": ([_vp, _vp, _sz, _int], _int),
    "lifeapi_weld_step_batch": ([_vp, _sz, _u32, _int], _int),
    "lifeapi_stable_pass_batch": ([_vp, _vp, _sz, _int, _u32, _int], _int),
    "lifeapi_neighbour_count_batch": ([_vp, _vp, _sz, _int], _int),
    "lifeapi_interaction_counts_batch": ([_vp, _vp, _sz, _int, _int], _int),
    "lifeapi_refined_step_batch": ([_vp, _vp, _sz, _int], _int),
    "lifeapi_contains_batch": ([_vp, _vp, _vp, _vp, _sz, _int], _int),
    "lifeapi_stable_vulnerable_batch_dev": ([_vp, _vp, _sz, _vp], _int),
    "lifeapi_stable_vulnerable_batch": ([_vp, _vp, _sz, _int], _int),
    "lifeapi_rle_lengths_batch_dev": ([_vp, _vp, _sz, _vp], _int),
    "lifeapi_rle_write_batch_dev": ([_vp, _vp, _vp, _sz, _vp], _int),
    "lifeapi_parse_rle_batch_dev": ([_vp, _vp, _sz, _vp, _vp, _vp], _int),
    "lifeapi_rle_batch": ([_vp, _sz, _vp, _sz, _vp, _int], _int),
    "lifeapi_parse_rle_batch": ([_vp, _vp, _sz, _vp, _vp, _int], _int),
    "lifeapi_match_batch_dev": ([_vp, _vp, _vp, _vp, _vp, _sz, _vp], _int),
    "lifeapi_convolve_batch_dev": ([_vp, _vp, _vp, _sz, _vp], _int),
    "lifeapi_interaction_offsets_batch_dev": ([_vp, _vp, _vp, _sz, _vp], _int),
    "lifeapi_match_batch": ([_vp, _vp, _vp, _vp, _vp, _sz, _int], _int),
    "lifeapi_convolve_batch": ([_vp, _vp, _vp, _sz, _int], _int),
    "lifeapi_interaction_offsets_batch": ([_vp, _vp, _vp, _sz, _int], _int),
    "lifeapi_transform_batch_dev": ([_vp, _vp, _sz, _u32, _int, _int, _vp], _int),
    "lifeapi_symmetricize_batch_dev": ([_vp, _vp, _sz, _u32, _int, _int, _vp], _int),
    "lifeapi_bounds_batch_dev": ([_vp, _vp, _sz, _vp], _int),
    "lifeapi_symmetry_orbit_batch_dev": ([_vp, _vp, _vp, _sz, _vp], _int),
    "lifeapi_transform_batch": ([_vp, _vp, _sz, _u32, _int, _int, _int], _int),
    "lifeapi_symmetricize_batch": ([_vp, _vp, _sz, _u32, _int, _int, _int], _int),
    "lifeapi_bounds_batch": ([_vp, _vp, _sz, _int], _int),
    "lifeapi_symmetry_orbit_batch": ([_vp, _vp, _vp, _sz, _int], _int),
    "lifeapi_transform_offsets_batch_dev": ([_vp, _vp, _sz, _u32, _vp, _vp], _int),
    "lifeapi_symmetricize_offsets_batch_dev": ([_vp, _vp, _sz, _u32, _vp, _vp], _int),
    "lifeapi_convolve_pair_batch_dev": ([_vp, _vp, _u32, _vp, _sz, _vp], _int),
    "lifeapi_intersecting_offsets_batch_dev": ([_vp, _vp, _u32, _vp, _sz, _vp], _int),
    "lifeapi_halve_batch_dev": ([_vp, _vp, _sz, _u32, _vp], _int),
    "lifeapi_skew_batch_dev": ([_vp, _vp, _sz, _int, _vp], _int),
    "lifeapi_transform_offsets_batch": ([_vp, _vp, _sz, _u32, _vp, _int], _int),
    "lifeapi_symmetricize_offsets_batch": ([_vp, _vp, _sz, _u32, _vp, _int], _int),
    "lifeapi_convolve_pair_batch": ([_vp, _vp, _u32, _vp, _sz, _int], _int),
    "lifeapi_intersecting_offsets_batch": ([_vp, _vp, _u32, _vp, _sz, _int], _int),
    "lifeapi_halve_batch": ([_vp, _vp, _sz, _u32, _int], _int),
    "lifeapi_skew_batch": ([_vp, _vp, _sz, _int, _int], _int),
    "lifeapi_first_on_batch_dev": ([_vp, _vp, _sz, _vp], _int),
    "lifeapi_component_containing_batch_dev": ([_vp, _vp, _int, _vp, _vp, _sz, _vp], _int),
    "lifeapi_components_batch_dev": ([_vp, _vp, _vp, _vp, _u32, _sz, _vp], _int),
    "lifeapi_first_on_batch": ([_vp, _vp, _sz, _int], _int),
    "lifeapi_component_containing_batch": ([_vp, _vp, _int, _vp, _vp, _sz, _int], _int),
    "lifeapi_components_batch": ([_vp, _vp, _vp, _vp, _u32, _sz, _int], _int),
    "lifeapi_weld_from_required_batch_dev": ([_vp, _vp, _int, _vp, _sz, _vp], _int),
    "lifeapi_weld_to_target_batch_dev": ([_vp, _vp, _vp, _sz, _vp], _int),
    "lifeapi_weld_to_stable_batch_dev": ([_vp, _vp, _int, _vp, _u32, _vp, _sz, _vp], _int),
    "lifeapi_weld_interaction_offsets_batch_dev": ([_vp, _vp, _vp, _sz, _vp], _int),
    "lifeapi_weld_from_required_batch": ([_vp, _vp, _int, _vp, _sz, _int], _int),
    "lifeapi_weld_to_target_batch": ([_vp, _vp, _vp, _sz, _int], _int),
    "lifeapi_weld_to_stable_batch": ([_vp, _vp, _int, _vp, _u32, _vp, _sz, _int], _int),
    "lifeapi_weld_interaction_offsets_batch": ([_vp, _vp, _vp, _sz, _int], _int),
    "lifeapi_stable_strip_pass_batch_dev": ([_vp, _vp, _vp, _sz, _int, _u32, _vp], _int),
    "lifeapi_stable_test_unknowns_batch_dev": ([_vp, _vp, _int, _vp, _sz, _u32, _vp], _int),
    "lifeapi_stable_propagate_and_test_batch_dev": ([_vp, _vp, _sz, _u32, _vp], _int),
    "lifeapi_stable_strip_pass_batch": ([_vp, _vp, _vp, _sz, _int, _u32, _int], _int),
    "lifeapi_stable_test_unknowns_batch": ([_vp, _vp, _int, _vp, _sz, _u32, _int], _int),
    "lifeapi_stable_propagate_and_test_batch": ([_vp, _vp, _sz, _u32, _int], _int),
    "lifeapi_stable_complete_workspace_bytes": ([_sz, _u32], _sz),
    "lifeapi_stable_complete_batch_dev": ([_vp, _vp, _int, _u32, ctypes.c_uint64, _u32, _vp, _vp, _vp, _sz, _vp, _sz,
                                           _vp], _int),
    "lifeapi_stable_complete_batch": ([_vp, _vp, _int, _u32, ctypes.c_uint64, _u32, _vp, _vp, _vp, _sz, _int], _int),
}
for _name, (_args, _res) in _SIGS.items():
    _f = getattr(lib, _name)
    _f.argtypes = _args
    _f.restype = _res

EXPORTS = tuple(_SIGS)


def _check(rc: int) -> None:
    if rc != 0:
        raise LifeApiError(rc, lib.lifeapi_last_error().decode(errors="replace"))


def abi_version() -> int:
    return lib.lifeapi_abi_version()


def device_count() -> int:
    return lib.lifeapi_device_count()


def step_kernel_name(generations: int = 1, n: int | None = None) -> str:
    """The shipped kernel configuration a step of `generations` runs on a
    batch of `n` universes (None: the name for batches of at most 4M)."""
    if n is None:
        return lib.lifeapi_step_kernel_name(generations).decode()
    return lib.lifeapi_step_kernel_name_n(generations, n).decode()


def _stream(stream) -> int:
    if stream is None:
        stream = torch.cuda.current_stream()
    return stream.cuda_stream if hasattr(stream, "cuda_stream") else int(stream)


def _planes(t: torch.Tensor, k: int, name: str) -> int:
    """n of a device tensor holding n universes of k 64-word planes each."""
    if not t.is_cuda:
        raise ValueError(f"{name} must be a device tensor")
    if t.dtype not in (torch.int64, torch.uint64) or not t.is_contiguous() or t.numel() % (k * N):
        shape = "(n, 64)" if k == 1 else f"(n, {k}*64)"
        raise ValueError(f"{name} must be a contiguous int64 tensor of shape {shape}")
    return t.numel() // (k * N)


def _universes(t: torch.Tensor, name: str = "states") -> int:
    return _planes(t, 1, name)


def empty_universes(n: int, device=None) -> torch.Tensor:
    return torch.empty((n, N), dtype=torch.int64, device=device or "cuda")


def step(states: torch.Tensor, out: torch.Tensor | None = None, generations: int = 1,
         stream=None) -> torch.Tensor:
    """Batched ``Stepped(generations)`` (LifeAPI.hpp:882-886); ``out`` may be ``states``."""
    n = _universes(states)
    if out is None:
        out = torch.empty_like(states)
    if _universes(out, "out") != n:
        raise ValueError("out has a different number of universes")
    _check(lib.lifeapi_step_batch_dev(states.data_ptr(), out.data_ptr(), n, generations, _stream(stream)))
    return out


def pop(states: torch.Tensor, stream=None) -> torch.Tensor:
    """Per-universe ``GetPop()`` (LifeAPI.hpp:290-298) as int32."""
    n = _universes(states)
    out = torch.empty(n, dtype=torch.int32, device=states.device)
    _check(lib.lifeapi_pop_batch_dev(states.data_ptr(), out.data_ptr(), n, _stream(stream)))
    return out


def hashes(states: torch.Tensor, stream=None) -> torch.Tensor:
    """Per-universe build-defined 64-bit hash (bit pattern in an int64 tensor)."""
    n = _universes(states)
    out = torch.empty(n, dtype=torch.int64, device=states.device)
    _check(lib.lifeapi_hash_batch_dev(states.data_ptr(), out.data_ptr(), n, _stream(stream)))
    return out


def contains(states: torch.Tensor, wanted: torch.Tensor, unwanted: torch.Tensor,
             stream=None) -> torch.Tensor:
    """Per-universe ``Contains(LifeTarget{wanted, unwanted})`` (LifeTarget.hpp:44-51)."""
    n = _universes(states)
    _universes(wanted, "wanted"), _universes(unwanted, "unwanted")
    out = torch.empty(n, dtype=torch.uint8, device=states.device)
    _check(lib.lifeapi_contains_batch_dev(states.data_ptr(), wanted.data_ptr(), unwanted.data_ptr(),
                                          out.data_ptr(), n, _stream(stream)))
    return out


def _out_like(states: torch.Tensor, out: torch.Tensor | None, n: int) -> torch.Tensor:
    if out is None:
        out = torch.empty_like(states)
    if _universes(out, "out") != n:
        raise ValueError("out has a different number of universes")
    return out


def match(states: torch.Tensor, wanted: torch.Tensor, unwanted: torch.Tensor,
          out: torch.Tensor | None = None, count: bool | str = False, stream=None):
    """Per-universe ``Match(LifeTarget{wanted, unwanted})`` (LifeTarget.hpp:53-55,
    LifeAPI.hpp:432-435): the mask of offsets at which the target is contained;
    ``out`` may be ``states``.  ``count=True`` returns (mask, int32 match
    counts), ``count="only"`` the counts alone (no mask is written)."""
    n = _universes(states)
    _universes(wanted, "wanted"), _universes(unwanted, "unwanted")
    only = count == "only"
    if only and out is not None:
        raise ValueError('count="only" writes no mask: out must be None')
    mask = None if only else _out_like(states, out, n)
    counts = torch.empty(n, dtype=torch.int32, device=states.device) if count else None
    _check(lib.lifeapi_match_batch_dev(states.data_ptr(), wanted.data_ptr(), unwanted.data_ptr(),
                                       None if only else mask.data_ptr(),
                                       counts.data_ptr() if count else None, n, _stream(stream)))
    return counts if only else (mask, counts) if count else mask


def convolve(states: torch.Tensor, pattern: torch.Tensor, out: torch.Tensor | None = None,
             stream=None) -> torch.Tensor:
    """Per-universe ``Convolve(pattern)`` (LifeAPI.hpp:1293-1370); ``out`` may be ``states``."""
    n = _universes(states)
    _universes(pattern, "pattern")
    out = _out_like(states, out, n)
    _check(lib.lifeapi_convolve_batch_dev(states.data_ptr(), pattern.data_ptr(), out.data_ptr(), n,
                                          _stream(stream)))
    return out


def interaction_offsets(states: torch.Tensor, other: torch.Tensor, out: torch.Tensor | None = None,
                        stream=None) -> torch.Tensor:
    """Per-universe ``InteractionOffsets(other)`` (LifeAPI.hpp:1066-1095); ``out`` may be ``states``."""
    n = _universes(states)
    _universes(other, "other")
    out = _out_like(states, out, n)
    _check(lib.lifeapi_interaction_offsets_batch_dev(states.data_ptr(), other.data_ptr(), out.data_ptr(), n,
                                                     _stream(stream)))
    return out


# SymmetryTransform and StaticSymmetry values (Symmetry.hpp:7-26, 57-79), the
# reference's enumerators in the reference's order
TRANSFORMS = ("Identity", "ReflectAcrossXEven", "ReflectAcrossX", "ReflectAcrossYEven", "ReflectAcrossY",
              "Rotate90Even", "Rotate90", "Rotate270Even", "Rotate270", "Rotate180OddBoth",
              "Rotate180EvenHorizontal", "Rotate180EvenVertical", "Rotate180EvenBoth", "ReflectAcrossYeqX",
              "ReflectAcrossYeqNegX", "ReflectAcrossYeqNegXP1")
SYMMETRIES = ("C1", "D2AcrossX", "D2AcrossXEven", "D2AcrossY", "D2AcrossYEven", "D2negdiagodd", "D2diagodd", "C2",
              "C2even", "C2verticaleven", "C2horizontaleven", "C4", "C4even", "D4", "D4even", "D4verticaleven",
              "D4horizontaleven", "D4diag", "D4diageven", "D8", "D8even")
# the transforms of SymmetryOrbit's eight images, in its order (Symmetry.hpp:801-803)
ORBIT_TRANSFORMS = (0, 2, 13, 4, 15, 6, 8, 9)


def _enum(v: int | str, names: tuple) -> int:
    return names.index(v) if isinstance(v, str) else int(v)


def transform(states: torch.Tensor, t: int | str, dx: int = 0, dy: int = 0, out: torch.Tensor | None = None,
              stream=None) -> torch.Tensor:
    """Per-universe ``Transformed(t).Moved(dx, dy)`` (Symmetry.hpp:105-173,
    LifeAPI.hpp:682-735); ``t`` a SymmetryTransform's value or name; ``out`` may be ``states``."""
    n = _universes(states)
    out = _out_like(states, out, n)
    _check(lib.lifeapi_transform_batch_dev(states.data_ptr(), out.data_ptr(), n, _enum(t, TRANSFORMS), dx, dy,
                                           _stream(stream)))
    return out


def symmetricize(states: torch.Tensor, symmetry: int | str, dx: int = 0, dy: int = 0,
                 out: torch.Tensor | None = None, stream=None) -> torch.Tensor:
    """Per-universe ``Symmetricize(state, symmetry, {dx, dy})`` (Symmetry.hpp:565-654);
    ``symmetry`` a StaticSymmetry's value or name; ``out`` may be ``states``."""
    n = _universes(states)
    out = _out_like(states, out, n)
    _check(lib.lifeapi_symmetricize_batch_dev(states.data_ptr(), out.data_ptr(), n, _enum(symmetry, SYMMETRIES),
                                              dx, dy, _stream(stream)))
    return out


def bounds(states: torch.Tensor, stream=None) -> torch.Tensor:
    """Per-universe ``XYBounds()`` (LifeAPI.hpp:446-484): (n, 4) int32 {left, top, right, bottom}."""
    n = _universes(states)
    out = torch.empty((n, 4), dtype=torch.int32, device=states.device)
    _check(lib.lifeapi_bounds_batch_dev(states.data_ptr(), out.data_ptr(), n, _stream(stream)))
    return out


def symmetry_orbit(states: torch.Tensor, images: bool = True, first: bool = True, stream=None):
    """Per-universe ``SymmetryOrbit`` / ``SymmetryOrbitRepresentatives``
    (Symmetry.hpp:798-830): the (n, 8, 64) normalised images in the order of
    ORBIT_TRANSFORMS and / or the uint8 mask whose bit i is set iff image i
    equals no earlier one (the set bits' images are the orbit)."""
    n = _universes(states)
    if not (images or first):
        raise ValueError("symmetry_orbit: nothing asked for")
    img = torch.empty((n, 8, N), dtype=torch.int64, device=states.device) if images else None
    fst = torch.empty(n, dtype=torch.uint8, device=states.device) if first else None
    _check(lib.lifeapi_symmetry_orbit_batch_dev(states.data_ptr(), img.data_ptr() if images else None,
                                                fst.data_ptr() if first else None, n, _stream(stream)))
    return (img, fst) if images and first else img if images else fst


# the transform IntersectingOffsets applies to pat1, by symmetry (Symmetry.hpp:733-767)
INTERSECTING_TRANSFORMS = {"C2": "Identity", "C4": "Rotate270", "D2AcrossX": "ReflectAcrossY",
                           "D2AcrossY": "ReflectAcrossX", "D2diagodd": "ReflectAcrossYeqNegXP1",
                           "D2negdiagodd": "ReflectAcrossYeqX"}
HALVE_MODES = ("Halve", "HalveX", "HalveY")


def _offsets(offsets: torch.Tensor, n: int) -> torch.Tensor:
    """(n, 2) int32 {dx, dy} on the device."""
    if not offsets.is_cuda or offsets.dtype != torch.int32 or not offsets.is_contiguous() or offsets.numel() != 2 * n:
        raise ValueError("offsets must be a contiguous int32 device tensor of shape (n, 2)")
    return offsets


def transform_offsets(states: torch.Tensor, t: int | str, offsets: torch.Tensor, out: torch.Tensor | None = None,
                      stream=None) -> torch.Tensor:
    """:func:`transform` with universe u moved by ``offsets[u]`` ((n, 2) int32); ``out`` may be ``states``."""
    n = _universes(states)
    out = _out_like(states, out, n)
    _check(lib.lifeapi_transform_offsets_batch_dev(states.data_ptr(), out.data_ptr(), n, _enum(t, TRANSFORMS),
                                                   _offsets(offsets, n).data_ptr(), _stream(stream)))
    return out


def symmetricize_offsets(states: torch.Tensor, symmetry: int | str, offsets: torch.Tensor,
                         out: torch.Tensor | None = None, stream=None) -> torch.Tensor:
    """:func:`symmetricize` with universe u taking ``offsets[u]`` ((n, 2) int32); ``out`` may be ``states``."""
    n = _universes(states)
    out = _out_like(states, out, n)
    _check(lib.lifeapi_symmetricize_offsets_batch_dev(states.data_ptr(), out.data_ptr(), n,
                                                      _enum(symmetry, SYMMETRIES), _offsets(offsets, n).data_ptr(),
                                                      _stream(stream)))
    return out


def convolve_pair(a: torch.Tensor, b: torch.Tensor | None = None, t: int | str = 0,
                  out: torch.Tensor | None = None, stream=None) -> torch.Tensor:
    """Per-universe ``a[u].Convolve(b[u].Transformed(t))`` (LifeAPI.hpp:1293-1370,
    Symmetry.hpp:105-173); ``b=None`` is ``a`` itself; ``out`` may be ``a`` or ``b``."""
    n = _universes(a, "a")
    b = a if b is None else b
    if _universes(b, "b") != n:
        raise ValueError("b has a different number of universes")
    out = _out_like(a, out, n)
    _check(lib.lifeapi_convolve_pair_batch_dev(a.data_ptr(), b.data_ptr(), _enum(t, TRANSFORMS), out.data_ptr(), n,
                                               _stream(stream)))
    return out


def intersecting_offsets(pat1: torch.Tensor, symmetry: int | str, pat2: torch.Tensor | None = None,
                         out: torch.Tensor | None = None, stream=None) -> torch.Tensor:
    """Per-universe ``IntersectingOffsets(pat1, pat2, symmetry)`` (Symmetry.hpp:729-768);
    ``pat2=None`` is ``IntersectingOffsets(active, symmetry)`` (Symmetry.hpp:770-772);
    ``symmetry`` a StaticSymmetry's value or name; ``out`` may be ``pat1`` or ``pat2``."""
    n = _universes(pat1, "pat1")
    pat2 = pat1 if pat2 is None else pat2
    if _universes(pat2, "pat2") != n:
        raise ValueError("pat2 has a different number of universes")
    out = _out_like(pat1, out, n)
    _check(lib.lifeapi_intersecting_offsets_batch_dev(pat1.data_ptr(), pat2.data_ptr(), _enum(symmetry, SYMMETRIES),
                                                      out.data_ptr(), n, _stream(stream)))
    return out


def halve(states: torch.Tensor, mode: int | str = 0, out: torch.Tensor | None = None, stream=None) -> torch.Tensor:
    """Per-universe ``Halve()`` (mode 0), ``HalveX()`` (1) or ``HalveY()`` (2)
    (Symmetry.hpp:681-709), by value or name; ``out`` may be ``states``."""
    n = _universes(states)
    out = _out_like(states, out, n)
    _check(lib.lifeapi_halve_batch_dev(states.data_ptr(), out.data_ptr(), n, _enum(mode, HALVE_MODES),
                                       _stream(stream)))
    return out


def skew(states: torch.Tensor, inverse: bool = False, out: torch.Tensor | None = None, stream=None) -> torch.Tensor:
    """Per-universe ``Skew()`` or, with ``inverse``, ``InvSkew()`` (Symmetry.hpp:711-727);
    ``out`` may be ``states``."""
    n = _universes(states)
    out = _out_like(states, out, n)
    _check(lib.lifeapi_skew_batch_dev(states.data_ptr(), out.data_ptr(), n, int(bool(inverse)), _stream(stream)))
    return out


def _corona(corona) -> np.ndarray | None:
    """The corona as the 64 host words the C ABI reads before it returns
    (None = the reference's default); a device tensor is brought to the host."""
    if corona is None:
        return None
    if isinstance(corona, torch.Tensor):
        corona = corona.cpu().numpy()
    c = np.ascontiguousarray(corona).view(np.uint64).reshape(-1)
    if c.size != N:
        raise ValueError("corona must be one universe of 64 words")
    return c


def first_on(states: torch.Tensor, stream=None) -> torch.Tensor:
    """Per-universe ``FirstOn()`` (LifeAPI.hpp:301-323): (n, 2) int32 {x, y}, the
    cell ``FirstCell()`` holds; (-1, -1) for the empty state."""
    n = _universes(states)
    out = torch.empty((n, 2), dtype=torch.int32, device=states.device)
    _check(lib.lifeapi_first_on_batch_dev(states.data_ptr(), out.data_ptr(), n, _stream(stream)))
    return out


def component_containing(states: torch.Tensor, seeds: torch.Tensor, corona=None, out: torch.Tensor | None = None,
                         stream=None) -> torch.Tensor:
    """Per-universe ``ComponentContaining(seed, corona)`` (LifeAPI.hpp:655-665).
    ``seeds`` holds one universe (the seed of the whole batch) or one per
    universe, told apart by its size (for a batch of one the two are the same
    thing); ``corona`` is host data (None = the reference's default); ``out`` may
    be ``states``, or ``seeds`` when per-universe."""
    n = _universes(states)
    k = _universes(seeds, "seeds")
    if k != 1 and k != n:
        raise ValueError("seeds must hold one universe or one per universe")
    out = _out_like(states, out, n)
    c = _corona(corona)
    _check(lib.lifeapi_component_containing_batch_dev(states.data_ptr(), seeds.data_ptr(), int(k == n),
                                                      None if c is None else c.ctypes.data, out.data_ptr(), n,
                                                      _stream(stream)))
    return out


def components(states: torch.Tensor, corona=None, max_components: int | None = None, count: bool = True,
               components_out: torch.Tensor | None = None, stream=None):
    """Per-universe ``Components(corona)`` (LifeAPI.hpp:667-676).  With
    ``max_components`` None only the int32 counts come back; otherwise the
    (n, max_components, 64) components in the reference's order, of which the
    first min(count, max_components) slots of a universe are written (the rest
    keep what ``components_out`` held, or are uninitialised), and with
    ``count`` the pair (components, counts).  The count is always the true
    one: count > max_components says the list was cut."""
    n = _universes(states)
    if max_components is None and not count:
        raise ValueError("components: nothing asked for")
    comps = None
    if max_components is not None:
        comps = components_out if components_out is not None else torch.empty(
            (n, max_components, N), dtype=torch.int64, device=states.device)
        if _universes(comps, "components_out") != n * max_components:
            raise ValueError("components_out must hold n x max_components universes")
    counts = torch.empty(n, dtype=torch.int32, device=states.device) if count else None
    c = _corona(corona)
    _check(lib.lifeapi_components_batch_dev(states.data_ptr(), None if c is None else c.ctypes.data,
                                            counts.data_ptr() if count else None,
                                            None if comps is None else comps.data_ptr(), max_components or 0, n,
                                            _stream(stream)))
    return counts if comps is None else (comps, counts) if count else comps


def step_contains(states: torch.Tensor, wanted: torch.Tensor, unwanted: torch.Tensor,
                  generations: int, final: torch.Tensor | None = None, stream=None):
    """First generation (1..gens, 0 = never) at which each universe contains the target."""
    n = _universes(states)
    first = torch.empty(n, dtype=torch.int32, device=states.device)
    fptr = 0 if final is None else final.data_ptr()
    if final is not None and _universes(final, "final") != n:
        raise ValueError("final has a different number of universes")
    _check(lib.lifeapi_step_contains_batch_dev(states.data_ptr(), fptr or None, wanted.data_ptr(),
                                               unwanted.data_ptr(), first.data_ptr(), n,
                                               generations, _stream(stream)))
    return first, final


def fill_random(n: int, seed: int, first_universe: int = 0, mode: int = 0,
                out: torch.Tensor | None = None, device=None, stream=None) -> torch.Tensor:
    """Seeded synthetic universes (see lifeapi_fill_random_dev)."""
    if out is None:
        out = empty_universes(n, device)
    if _universes(out, "out") != n:
        raise ValueError("out has a different number of universes")
    _check(lib.lifeapi_fill_random_dev(out.data_ptr(), n, seed & (2**64 - 1), first_universe,
                                       mode, _stream(stream)))
    return out


def _host_u64(a: np.ndarray) -> np.ndarray:
    a = np.ascontiguousarray(a, dtype=np.uint64)
    if a.size % N:
        raise ValueError("host batch must hold whole universes (multiples of 64 words)")
    return a


def step_host(states: np.ndarray, generations: int = 1, device: int = 0,
              out: np.ndarray | None = None) -> np.ndarray:
    """Host-pointer ``lifeapi_step_batch`` (synchronous, PCIe-staged)."""
    src = _host_u64(states)
    dst = np.empty_like(src) if out is None else out
    _check(lib.lifeapi_step_batch(src.ctypes.data, dst.ctypes.data, src.size // N, generations, device))
    return dst


def step_contains_host(states: np.ndarray, wanted: np.ndarray, unwanted: np.ndarray, generations: int,
                       final: np.ndarray | None = None, device: int = 0) -> np.ndarray:
    """Host-pointer ``lifeapi_step_contains_batch``: first generation (1..gens,
    0 = never) containing the target; ``final`` (may be ``states``) gets
    Stepped(gens)."""
    src = _host_u64(states)
    w, u = _host_u64(wanted), _host_u64(unwanted)
    first = np.empty(src.size // N, dtype=np.uint32)
    fptr = None if final is None else final.ctypes.data
    _check(lib.lifeapi_step_contains_batch(src.ctypes.data, fptr, w.ctypes.data, u.ctypes.data,
                                           first.ctypes.data, src.size // N, generations, device))
    return first


def match_host(states: np.ndarray, wanted: np.ndarray, unwanted: np.ndarray, out: np.ndarray | None = None,
               count: bool | str = False, device: int = 0):
    """Host-pointer ``lifeapi_match_batch``; ``out`` and ``count`` as :func:`match`."""
    src, w, u = _host_u64(states), _host_u64(wanted), _host_u64(unwanted)
    n, only = src.size // N, count == "only"
    mask = None if only else (np.empty_like(src) if out is None else out)
    counts = np.empty(n, dtype=np.uint32) if count else None
    _check(lib.lifeapi_match_batch(src.ctypes.data, w.ctypes.data, u.ctypes.data,
                                   None if only else mask.ctypes.data,
                                   counts.ctypes.data if count else None, n, device))
    return counts if only else (mask, counts) if count else mask


def convolve_host(states: np.ndarray, pattern: np.ndarray, out: np.ndarray | None = None,
                  device: int = 0) -> np.ndarray:
    """Host-pointer ``lifeapi_convolve_batch``."""
    src, p = _host_u64(states), _host_u64(pattern)
    dst = np.empty_like(src) if out is None else out
    _check(lib.lifeapi_convolve_batch(src.ctypes.data, p.ctypes.data, dst.ctypes.data, src.size // N, device))
    return dst


def interaction_offsets_host(states: np.ndarray, other: np.ndarray, out: np.ndarray | None = None,
                             device: int = 0) -> np.ndarray:
    """Host-pointer ``lifeapi_interaction_offsets_batch``."""
    src, p = _host_u64(states), _host_u64(other)
    dst = np.empty_like(src) if out is None else out
    _check(lib.lifeapi_interaction_offsets_batch(src.ctypes.data, p.ctypes.data, dst.ctypes.data, src.size // N,
                                                 device))
    return dst


def transform_host(states: np.ndarray, t: int | str, dx: int = 0, dy: int = 0, out: np.ndarray | None = None,
                   device: int = 0) -> np.ndarray:
    """Host-pointer ``lifeapi_transform_batch``."""
    src = _host_u64(states)
    dst = np.empty_like(src) if out is None else out
    _check(lib.lifeapi_transform_batch(src.ctypes.data, dst.ctypes.data, src.size // N, _enum(t, TRANSFORMS), dx, dy,
                                       device))
    return dst


def symmetricize_host(states: np.ndarray, symmetry: int | str, dx: int = 0, dy: int = 0,
                      out: np.ndarray | None = None, device: int = 0) -> np.ndarray:
    """Host-pointer ``lifeapi_symmetricize_batch``."""
    src = _host_u64(states)
    dst = np.empty_like(src) if out is None else out
    _check(lib.lifeapi_symmetricize_batch(src.ctypes.data, dst.ctypes.data, src.size // N,
                                          _enum(symmetry, SYMMETRIES), dx, dy, device))
    return dst


def bounds_host(states: np.ndarray, device: int = 0) -> np.ndarray:
    """Host-pointer ``lifeapi_bounds_batch``: (n, 4) int32."""
    src = _host_u64(states)
    out = np.empty((src.size // N, 4), dtype=np.int32)
    _check(lib.lifeapi_bounds_batch(src.ctypes.data, out.ctypes.data, src.size // N, device))
    return out


def symmetry_orbit_host(states: np.ndarray, images: bool = True, first: bool = True, device: int = 0):
    """Host-pointer ``lifeapi_symmetry_orbit_batch``; results as :func:`symmetry_orbit`."""
    src = _host_u64(states)
    n = src.size // N
    if not (images or first):
        raise ValueError("symmetry_orbit_host: nothing asked for")
    img = np.empty((n, 8, N), dtype=np.uint64) if images else None
    fst = np.empty(n, dtype=np.uint8) if first else None
    _check(lib.lifeapi_symmetry_orbit_batch(src.ctypes.data, img.ctypes.data if images else None,
                                            fst.ctypes.data if first else None, n, device))
    return (img, fst) if images and first else img if images else fst


def _host_offsets(offsets: np.ndarray, n: int) -> np.ndarray:
    o = np.ascontiguousarray(offsets, dtype=np.int32)
    if o.size != 2 * n:
        raise ValueError("offsets must hold n x {dx, dy}")
    return o


def transform_offsets_host(states: np.ndarray, t: int | str, offsets: np.ndarray, out: np.ndarray | None = None,
                           device: int = 0) -> np.ndarray:
    """Host-pointer ``lifeapi_transform_offsets_batch``."""
    src = _host_u64(states)
    o = _host_offsets(offsets, src.size // N)
    dst = np.empty_like(src) if out is None else out
    _check(lib.lifeapi_transform_offsets_batch(src.ctypes.data, dst.ctypes.data, src.size // N,
                                               _enum(t, TRANSFORMS), o.ctypes.data, device))
    return dst


def symmetricize_offsets_host(states: np.ndarray, symmetry: int | str, offsets: np.ndarray,
                              out: np.ndarray | None = None, device: int = 0) -> np.ndarray:
    """Host-pointer ``lifeapi_symmetricize_offsets_batch``."""
    src = _host_u64(states)
    o = _host_offsets(offsets, src.size // N)
    dst = np.empty_like(src) if out is None else out
    _check(lib.lifeapi_symmetricize_offsets_batch(src.ctypes.data, dst.ctypes.data, src.size // N,
                                                  _enum(symmetry, SYMMETRIES), o.ctypes.data, device))
    return dst


def _host_pair(a: np.ndarray, b: np.ndarray | None) -> tuple:
    x = _host_u64(a)
    y = x if b is None or b is a else _host_u64(b)
    if y.size != x.size:
        raise ValueError("the operands hold different numbers of universes")
    return x, y


def convolve_pair_host(a: np.ndarray, b: np.ndarray | None = None, t: int | str = 0, out: np.ndarray | None = None,
                       device: int = 0) -> np.ndarray:
    """Host-pointer ``lifeapi_convolve_pair_batch``; ``b=None`` is ``a`` itself."""
    x, y = _host_pair(a, b)
    dst = np.empty_like(x) if out is None else out
    _check(lib.lifeapi_convolve_pair_batch(x.ctypes.data, y.ctypes.data, _enum(t, TRANSFORMS), dst.ctypes.data,
                                           x.size // N, device))
    return dst


def intersecting_offsets_host(pat1: np.ndarray, symmetry: int | str, pat2: np.ndarray | None = None,
                              out: np.ndarray | None = None, device: int = 0) -> np.ndarray:
    """Host-pointer ``lifeapi_intersecting_offsets_batch``; ``pat2=None`` is ``pat1`` itself."""
    x, y = _host_pair(pat1, pat2)
    dst = np.empty_like(x) if out is None else out
    _check(lib.lifeapi_intersecting_offsets_batch(x.ctypes.data, y.ctypes.data, _enum(symmetry, SYMMETRIES),
                                                  dst.ctypes.data, x.size // N, device))
    return dst


def halve_host(states: np.ndarray, mode: int | str = 0, out: np.ndarray | None = None, device: int = 0) -> np.ndarray:
    """Host-pointer ``lifeapi_halve_batch``."""
    src = _host_u64(states)
    dst = np.empty_like(src) if out is None else out
    _check(lib.lifeapi_halve_batch(src.ctypes.data, dst.ctypes.data, src.size // N, _enum(mode, HALVE_MODES), device))
    return dst


def skew_host(states: np.ndarray, inverse: bool = False, out: np.ndarray | None = None,
              device: int = 0) -> np.ndarray:
    """Host-pointer ``lifeapi_skew_batch``."""
    src = _host_u64(states)
    dst = np.empty_like(src) if out is None else out
    _check(lib.lifeapi_skew_batch(src.ctypes.data, dst.ctypes.data, src.size // N, int(bool(inverse)), device))
    return dst


def first_on_host(states: np.ndarray, device: int = 0) -> np.ndarray:
    """Host-pointer ``lifeapi_first_on_batch``: (n, 2) int32."""
    src = _host_u64(states)
    out = np.empty((src.size // N, 2), dtype=np.int32)
    _check(lib.lifeapi_first_on_batch(src.ctypes.data, out.ctypes.data, src.size // N, device))
    return out


def component_containing_host(states: np.ndarray, seeds: np.ndarray, corona=None, out: np.ndarray | None = None,
                              device: int = 0) -> np.ndarray:
    """Host-pointer ``lifeapi_component_containing_batch``; ``seeds`` and ``out`` as :func:`component_containing`."""
    src, sd = _host_u64(states), _host_u64(seeds)
    n = src.size // N
    if sd.size != N and sd.size != src.size:
        raise ValueError("seeds must hold one universe or one per universe")
    dst = np.empty_like(src) if out is None else out
    c = _corona(corona)
    _check(lib.lifeapi_component_containing_batch(src.ctypes.data, sd.ctypes.data, int(sd.size == src.size),
                                                  None if c is None else c.ctypes.data, dst.ctypes.data, n, device))
    return dst


def components_host(states: np.ndarray, corona=None, max_components: int | None = None, count: bool = True,
                    components_out: np.ndarray | None = None, device: int = 0):
    """Host-pointer ``lifeapi_components_batch``; results as :func:`components`."""
    src = _host_u64(states)
    n = src.size // N
    if max_components is None and not count:
        raise ValueError("components_host: nothing asked for")
    comps = None
    if max_components is not None:
        comps = np.empty((n, max_components, N), dtype=np.uint64) if components_out is None else components_out
    counts = np.empty(n, dtype=np.uint32) if count else None
    c = _corona(corona)
    _check(lib.lifeapi_components_batch(src.ctypes.data, None if c is None else c.ctypes.data,
                                        counts.ctypes.data if count else None,
                                        None if comps is None else comps.ctypes.data, max_components or 0, n, device))
    return counts if comps is None else (comps, counts) if count else comps


class host_pinned:
    """Context manager: page-lock numpy arrays (lifeapi_host_register) for
    the host-pointer calls inside the block."""

    def __init__(self, *arrays: np.ndarray):
        self.arrays = arrays

    def __enter__(self):
        done = []
        try:
            for a in self.arrays:
                _check(lib.lifeapi_host_register(a.ctypes.data, a.nbytes))
                done.append(a)
        except Exception:
            for a in done:
                lib.lifeapi_host_unregister(a.ctypes.data)
            raise
        return self

    def __exit__(self, *exc):
        for a in self.arrays:
            _check(lib.lifeapi_host_unregister(a.ctypes.data))
        return False


def pop_host(states: np.ndarray, device: int = 0) -> np.ndarray:
    src = _host_u64(states)
    out = np.empty(src.size // N, dtype=np.uint32)
    _check(lib.lifeapi_pop_batch(src.ctypes.data, out.ctypes.data, src.size // N, device))
    return out


def loaded_hip_runtimes() -> list[str]:
    """Paths of every libamdhip64 mapped into this process (must be exactly one)."""
    paths = set()
    with open("/proc/self/maps") as f:
        for line in f:
            p = line.split()[-1] if len(line.split()) >= 6 else ""
            if "libamdhip64" in p:
                paths.add(p)
    return sorted(paths)


def refined_step(planes: torch.Tensor, out: torch.Tensor | None = None, stream=None) -> torch.Tensor:
    """Config-5 ternary step: (n, 11*64) int64 planes -> (n, 3*64) planes
    (see lifeapi_refined_step_batch_dev)."""
    n = _planes(planes, 11, "planes")
    if out is None:
        out = torch.empty((n, 3 * N), dtype=torch.int64, device=planes.device)
    _check(lib.lifeapi_refined_step_batch_dev(planes.data_ptr(), out.data_ptr(), n, _stream(stream)))
    return out


def weld_step(welds: torch.Tensor, generations: int = 1, stream=None) -> torch.Tensor:
    """LifeWeld::Step()^generations in place on (n, 4*64) {state, frozen2,
    frozen1, frozen0} planes (LifeWeld.hpp:169-186)."""
    _check(lib.lifeapi_weld_step_batch_dev(welds.data_ptr(), _planes(welds, 4, "welds"), generations,
                                           _stream(stream)))
    return welds


def _one_or_n(t: torch.Tensor, n: int, name: str) -> int:
    """1 if t holds one universe per object of the batch, 0 if one for all"""
    k = _universes(t, name)
    if k != 1 and k != n:
        raise ValueError(f"{name} must hold one universe or one per object")
    return int(k == n and n != 1)


def _out_planes(out: torch.Tensor | None, n: int, k: int, like: torch.Tensor, name: str) -> torch.Tensor:
    if out is None:
        return torch.empty((n, k * N), dtype=torch.int64, device=like.device)
    if _planes(out, k, name) != n:
        raise ValueError(f"{name} has a different number of objects")
    return out


def weld_from_required(states: torch.Tensor, required: torch.Tensor, out: torch.Tensor | None = None,
                       stream=None) -> torch.Tensor:
    """Per-universe ``LifeWeld::FromRequired(state, required)`` (LifeWeld.hpp:
    133-159): (n, 4*64) {state, frozen2, frozen1, frozen0}.  ``required`` holds
    one universe for the whole batch or one per universe."""
    n = _universes(states)
    per = _one_or_n(required, n, "required")
    out = _out_planes(out, n, 4, states, "out")
    _check(lib.lifeapi_weld_from_required_batch_dev(states.data_ptr(), required.data_ptr(), per, out.data_ptr(), n,
                                                    _stream(stream)))
    return out


def weld_to_target(welds: torch.Tensor, wanted: torch.Tensor | None = None, unwanted: torch.Tensor | None = None,
                   stream=None) -> tuple[torch.Tensor, torch.Tensor]:
    """Per-weld ``ToTarget()`` (LifeWeld.hpp:188-191): (wanted, unwanted), (n, 64) each."""
    n = _planes(welds, 4, "welds")
    wanted = _out_planes(wanted, n, 1, welds, "wanted")
    unwanted = _out_planes(unwanted, n, 1, welds, "unwanted")
    _check(lib.lifeapi_weld_to_target_batch_dev(welds.data_ptr(), wanted.data_ptr(), unwanted.data_ptr(), n,
                                                _stream(stream)))
    return wanted, unwanted


def weld_to_stable(welds: torch.Tensor, active: torch.Tensor | None = None, duration: int = 0,
                   mask: torch.Tensor | None = None, out: torch.Tensor | None = None, stream=None) -> torch.Tensor:
    """Per-weld ``ToStable(active, duration, mask)`` (LifeWeld.hpp:279-400) as
    (n, 10*64) LifeStable planes, the layout :func:`stable_pass` takes.
    ``active``: None (empty), one universe or one per weld; ``mask``: None (all
    cells, the reference's default) or one universe.  ``duration == 0`` is
    ``ToStable()``."""
    n = _planes(welds, 4, "welds")
    per = 0 if active is None else _one_or_n(active, n, "active")
    if mask is not None and _universes(mask, "mask") != 1:
        raise ValueError("mask must hold one universe")
    out = _out_planes(out, n, 10, welds, "out")
    _check(lib.lifeapi_weld_to_stable_batch_dev(welds.data_ptr(), None if active is None else active.data_ptr(), per,
                                                None if mask is None else mask.data_ptr(), duration, out.data_ptr(),
                                                n, _stream(stream)))
    return out


def weld_interaction_offsets(welds: torch.Tensor, other: torch.Tensor, out: torch.Tensor | None = None,
                             stream=None) -> torch.Tensor:
    """Per-weld ``InteractionOffsets(other)`` (LifeWeld.hpp:206-245), ``other`` one
    LifeWeld of 4*64 words: (n, 64)."""
    n = _planes(welds, 4, "welds")
    if _planes(other, 4, "other") != 1:
        raise ValueError("other must hold one LifeWeld (4*64 words)")
    out = _out_planes(out, n, 1, welds, "out")
    _check(lib.lifeapi_weld_interaction_offsets_batch_dev(welds.data_ptr(), other.data_ptr(), out.data_ptr(), n,
                                                          _stream(stream)))
    return out


def _host_planes(a: np.ndarray, k: int, name: str) -> tuple[np.ndarray, int]:
    a = np.ascontiguousarray(a, dtype=np.uint64)
    if a.size % (k * N):
        raise ValueError(f"{name} must hold whole objects of {k}*64 words")
    return a, a.size // (k * N)


def weld_from_required_host(states: np.ndarray, required: np.ndarray, device: int = 0) -> np.ndarray:
    """Host-pointer ``lifeapi_weld_from_required_batch``."""
    src, req = _host_u64(states), _host_u64(required)
    n, k = src.size // N, req.size // N
    if k != 1 and k != n:
        raise ValueError("required must hold one universe or one per universe")
    out = np.empty((n, 4 * N), dtype=np.uint64)
    _check(lib.lifeapi_weld_from_required_batch(src.ctypes.data, req.ctypes.data, int(k == n and n != 1),
                                                out.ctypes.data, n, device))
    return out


def weld_to_target_host(welds: np.ndarray, device: int = 0) -> tuple[np.ndarray, np.ndarray]:
    """Host-pointer ``lifeapi_weld_to_target_batch``."""
    src, n = _host_planes(welds, 4, "welds")
    wanted, unwanted = np.empty((n, N), dtype=np.uint64), np.empty((n, N), dtype=np.uint64)
    _check(lib.lifeapi_weld_to_target_batch(src.ctypes.data, wanted.ctypes.data, unwanted.ctypes.data, n, device))
    return wanted, unwanted


def weld_to_stable_host(welds: np.ndarray, active: np.ndarray | None = None, duration: int = 0,
                        mask: np.ndarray | None = None, device: int = 0) -> np.ndarray:
    """Host-pointer ``lifeapi_weld_to_stable_batch``."""
    src, n = _host_planes(welds, 4, "welds")
    act = None if active is None else _host_u64(active)
    msk = None if mask is None else _host_u64(mask)
    if act is not None and act.size // N not in (1, n):
        raise ValueError("active must hold one universe or one per weld")
    if msk is not None and msk.size != N:
        raise ValueError("mask must hold one universe")
    out = np.empty((n, 10 * N), dtype=np.uint64)
    _check(lib.lifeapi_weld_to_stable_batch(src.ctypes.data, None if act is None else act.ctypes.data,
                                            int(act is not None and act.size // N == n and n != 1),
                                            None if msk is None else msk.ctypes.data, duration, out.ctypes.data, n,
                                            device))
    return out


def weld_interaction_offsets_host(welds: np.ndarray, other: np.ndarray, device: int = 0) -> np.ndarray:
    """Host-pointer ``lifeapi_weld_interaction_offsets_batch``."""
    src, n = _host_planes(welds, 4, "welds")
    oth, k = _host_planes(other, 4, "other")
    if k != 1:
        raise ValueError("other must hold one LifeWeld (4*64 words)")
    out = np.empty((n, N), dtype=np.uint64)
    _check(lib.lifeapi_weld_interaction_offsets_batch(src.ctypes.data, oth.ctypes.data, out.ctypes.data, n, device))
    return out


STABLE_PASSES = ("sync", "options", "signal", "step", "propagate", "stabilise")


def stable_pass(planes: torch.Tensor, which: str | int, max_iters: int = 0,
                stream=None) -> torch.Tensor:
    """LifeStable pass in place on (n, 10*64) planes; returns uint8 flags
    (bit0 consistent, bit1 changed, bit2 stopped by max_iters)."""
    w = STABLE_PASSES.index(which) if isinstance(which, str) else int(which)
    n = _planes(planes, 10, "planes")
    flags = torch.empty(n, dtype=torch.uint8, device=planes.device)
    _check(lib.lifeapi_stable_pass_batch_dev(planes.data_ptr(), flags.data_ptr(), n, w, max_iters,
                                             _stream(stream)))
    return flags


def stable_vulnerable(planes: torch.Tensor, stream=None) -> torch.Tensor:
    """LifeStable::Vulnerable() (LifeStable.hpp:366-412) of (n, 10*64) planes -> (n, 64)."""
    n = _planes(planes, 10, "planes")
    out = torch.empty((n, N), dtype=torch.int64, device=planes.device)
    _check(lib.lifeapi_stable_vulnerable_batch_dev(planes.data_ptr(), out.data_ptr(), n, _stream(stream)))
    return out


STABLE_STRIP_PASSES = ("sync_strip", "options_strip", "signal_strip", "step_strip", "propagate_strip",
                       "stabilise_strip")


def _strip_pass(which: str | int) -> int:
    w = STABLE_STRIP_PASSES.index(which) if isinstance(which, str) else int(which)
    if not 0 <= w < 6:
        raise ValueError("which must name one of STABLE_STRIP_PASSES")
    return w


def stable_strip_pass(planes: torch.Tensor, columns: torch.Tensor, which: str | int, max_iters: int = 0,
                      stream=None) -> torch.Tensor:
    """LifeStable strip pass (LifeStable.hpp:921-948, 995-1249) in place on (n,
    10*64) planes, object u at column ``columns[u]`` (uint8, 0..63); returns
    uint8 flags (bit0 consistent, bit1 changed, bit2 stopped by max_iters)."""
    w = _strip_pass(which)
    n = _planes(planes, 10, "planes")
    if not columns.is_cuda or columns.dtype != torch.uint8 or not columns.is_contiguous() or columns.numel() != n:
        raise ValueError("columns must be a contiguous uint8 device tensor with one column per object")
    flags = torch.empty(n, dtype=torch.uint8, device=planes.device)
    _check(lib.lifeapi_stable_strip_pass_batch_dev(planes.data_ptr(), columns.data_ptr(), flags.data_ptr(), n, w,
                                                   max_iters, _stream(stream)))
    return flags


def stable_test_unknowns(planes: torch.Tensor, cells: torch.Tensor, max_iters: int = 0, stream=None) -> torch.Tensor:
    """``TestUnknowns(cells)`` (LifeStable.hpp:1321-1338) in place on (n, 10*64)
    planes; ``cells`` holds one universe for the whole batch or one per object.
    Returns uint8 flags: consistent | changed << 1, or 4 where ``max_iters``
    stopped a PropagateStrip (that object is then left as it was)."""
    n = _planes(planes, 10, "planes")
    per = _one_or_n(cells, n, "cells")
    flags = torch.empty(n, dtype=torch.uint8, device=planes.device)
    _check(lib.lifeapi_stable_test_unknowns_batch_dev(planes.data_ptr(), cells.data_ptr(), per, flags.data_ptr(), n,
                                                      max_iters, _stream(stream)))
    return flags


def stable_propagate_and_test(planes: torch.Tensor, max_iters: int = 0, stream=None) -> torch.Tensor:
    """``PropagateAndTest()`` (LifeStable.hpp:163-184) in place on (n, 10*64)
    planes: Propagate, then TestUnknowns(Vulnerable().ZOI()), until neither
    changes.  Returns uint8 flags: consistent | changed << 1, or 4 where
    ``max_iters`` stopped a loop (that object is then left as it was)."""
    n = _planes(planes, 10, "planes")
    flags = torch.empty(n, dtype=torch.uint8, device=planes.device)
    _check(lib.lifeapi_stable_propagate_and_test_batch_dev(planes.data_ptr(), flags.data_ptr(), n, max_iters,
                                                           _stream(stream)))
    return flags


def stable_strip_pass_host(planes: np.ndarray, columns: np.ndarray, which: str | int, max_iters: int = 0,
                           device: int = 0) -> tuple[np.ndarray, np.ndarray]:
    """Host-pointer ``lifeapi_stable_strip_pass_batch``: (planes, flags), the input untouched."""
    w = _strip_pass(which)
    src, n = _host_planes(planes, 10, "planes")
    col = np.ascontiguousarray(columns, dtype=np.uint8)
    if col.size != n:
        raise ValueError("columns must hold one column per object")
    out, flags = src.reshape(n, 10 * N).copy(), np.empty(n, dtype=np.uint8)
    _check(lib.lifeapi_stable_strip_pass_batch(out.ctypes.data, col.ctypes.data, flags.ctypes.data, n, w, max_iters,
                                               device))
    return out, flags


def stable_test_unknowns_host(planes: np.ndarray, cells: np.ndarray, max_iters: int = 0,
                              device: int = 0) -> tuple[np.ndarray, np.ndarray]:
    """Host-pointer ``lifeapi_stable_test_unknowns_batch``: (planes, flags), the input untouched."""
    src, n = _host_planes(planes, 10, "planes")
    cel = _host_u64(cells)
    if cel.size // N not in (1, n):
        raise ValueError("cells must hold one universe or one per object")
    out, flags = src.reshape(n, 10 * N).copy(), np.empty(n, dtype=np.uint8)
    _check(lib.lifeapi_stable_test_unknowns_batch(out.ctypes.data, cel.ctypes.data, int(cel.size // N == n and n != 1),
                                                  flags.ctypes.data, n, max_iters, device))
    return out, flags


def stable_propagate_and_test_host(planes: np.ndarray, max_iters: int = 0,
                                   device: int = 0) -> tuple[np.ndarray, np.ndarray]:
    """Host-pointer ``lifeapi_stable_propagate_and_test_batch``: (planes, flags), the input untouched."""
    src, n = _host_planes(planes, 10, "planes")
    out, flags = src.reshape(n, 10 * N).copy(), np.empty(n, dtype=np.uint8)
    _check(lib.lifeapi_stable_propagate_and_test_batch(out.ctypes.data, flags.ctypes.data, n, max_iters, device))
    return out, flags


COMPLETE_MINIMISE, COMPLETE_USE_SEED = 1, 2
COMPLETION_RESULTS = ("completed", "inconsistent", "timeout", "too_deep", "bad_seed")
# what stable_complete allocates at most when it is given no workspace
COMPLETE_WORKSPACE_CAP = 1 << 30


def stable_complete_workspace_bytes(n: int, max_depth: int = 64) -> int:
    """Bytes of workspace a full grid of ``stable_complete`` searches uses for
    ``n`` objects on the current device (one stack of ``max_depth`` frames per
    resident wave); any size holding one stack is accepted."""
    b = lib.lifeapi_stable_complete_workspace_bytes(n, max_depth)
    if b == 0:
        raise LifeApiError(-1, lib.lifeapi_last_error().decode(errors="replace"))
    return b


def stable_complete(planes: torch.Tensor, *, minimise: bool = False, seed: torch.Tensor | None = None,
                    node_budget: int = 0, max_depth: int = 64, workspace: torch.Tensor | None = None,
                    stream=None) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``CompleteStable(minimise, seed is not None, seed)`` (LifeStable.hpp:
    1340-1458) of (n, 10*64) planes, which are not written, with a per-object
    node budget (0 = 65536) in place of the reference's clock: (result uint8,
    best (n, 64), nodes int64).  result: 0 completed, 1 inconsistent, 2
    timeout, 3 more than ``max_depth`` frames, 4 empty seed; best is empty
    unless completed.  ``seed``: one universe or one per object.  ``workspace``:
    a device tensor of at least one stack (``stable_complete_workspace_bytes(1,
    max_depth)``), 128-byte aligned; None allocates one (at most 1 GiB)."""
    n = _planes(planes, 10, "planes")
    per = 0 if seed is None else _one_or_n(seed, n, "seed")
    flags = (COMPLETE_MINIMISE if minimise else 0) | (COMPLETE_USE_SEED if seed is not None else 0)
    result = torch.empty(n, dtype=torch.uint8, device=planes.device)
    best = torch.empty((n, N), dtype=torch.int64, device=planes.device)
    nodes = torch.empty(n, dtype=torch.int64, device=planes.device)
    if n == 0:
        return result, best, nodes
    if workspace is None:
        with torch.cuda.device(planes.device):
            want = min(stable_complete_workspace_bytes(n, max_depth),
                       max(COMPLETE_WORKSPACE_CAP, stable_complete_workspace_bytes(1, max_depth)))
        workspace = torch.empty(want, dtype=torch.uint8, device=planes.device)
    elif not workspace.is_cuda or not workspace.is_contiguous():
        raise ValueError("workspace must be a contiguous device tensor")
    _check(lib.lifeapi_stable_complete_batch_dev(planes.data_ptr(), None if seed is None else seed.data_ptr(), per,
                                                 flags, node_budget, max_depth, best.data_ptr(), result.data_ptr(),
                                                 nodes.data_ptr(), n, workspace.data_ptr(),
                                                 workspace.numel() * workspace.element_size(), _stream(stream)))
    return result, best, nodes


def stable_complete_host(planes: np.ndarray, *, minimise: bool = False, seed: np.ndarray | None = None,
                         node_budget: int = 0, max_depth: int = 64,
                         device: int = 0) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Host-pointer ``lifeapi_stable_complete_batch``: (result, best, nodes)."""
    src, n = _host_planes(planes, 10, "planes")
    sd = None if seed is None else _host_u64(seed)
    if sd is not None and sd.size // N not in (1, n):
        raise ValueError("seed must hold one universe or one per object")
    flags = (COMPLETE_MINIMISE if minimise else 0) | (COMPLETE_USE_SEED if sd is not None else 0)
    result, best, nodes = np.empty(n, np.uint8), np.empty((n, N), np.uint64), np.empty(n, np.uint64)
    _check(lib.lifeapi_stable_complete_batch(src.ctypes.data, None if sd is None else sd.ctypes.data,
                                             int(sd is not None and sd.size // N == n and n != 1), flags, node_budget,
                                             max_depth, best.ctypes.data, result.ctypes.data, nodes.ctypes.data, n,
                                             device))
    return result, best, nodes


def neighbour_count(states: torch.Tensor, stream=None) -> torch.Tensor:
    """NeighbourCount planes (NeighbourCount.hpp:40-70): (n, 4, 64) = bit3..bit0."""
    n = _universes(states)
    out = torch.empty((n, 4, N), dtype=torch.int64, device=states.device)
    _check(lib.lifeapi_neighbour_count_batch_dev(states.data_ptr(), out.data_ptr(), n, _stream(stream)))
    return out


def interaction_counts(states: torch.Tensor, with_next: bool = False, stream=None) -> torch.Tensor:
    """InteractionCounts[AndNext] (LifeAPI.hpp:956-1040): (n, 3|4, 64) planes
    out1, out2, outMore[, next]."""
    n = _universes(states)
    out = torch.empty((n, 4 if with_next else 3, N), dtype=torch.int64, device=states.device)
    _check(lib.lifeapi_interaction_counts_batch_dev(states.data_ptr(), out.data_ptr(), n,
                                                    1 if with_next else 0, _stream(stream)))
    return out


def rle(states: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """``LifeState::RLE()`` (Parsing.hpp:8-63,200-204) of every universe on
    the device, on torch's current stream: (text uint8 tensor, offsets int64
    tensor of n+1; pattern u = text[offsets[u]:offsets[u+1]])."""
    n = _universes(states)
    s = _stream(None)
    lens = torch.empty(n, dtype=torch.int32, device=states.device)
    _check(lib.lifeapi_rle_lengths_batch_dev(states.data_ptr(), lens.data_ptr(), n, s))
    offs = torch.zeros(n + 1, dtype=torch.int64, device=states.device)
    if n:
        torch.cumsum(lens, 0, out=offs[1:])
    total = int(offs[-1].item()) if n else 0
    text = torch.empty(max(total, 1), dtype=torch.uint8, device=states.device)
    _check(lib.lifeapi_rle_write_batch_dev(states.data_ptr(), offs.data_ptr(), text.data_ptr(), n, s))
    return text[:total], offs


def parse_rle(text: torch.Tensor, offsets: torch.Tensor, stream=None) -> tuple[torch.Tensor, torch.Tensor]:
    """``LifeState::Parse`` (Parsing.hpp:143-198) of every pattern of a device
    text blob: (states (n, 64) int64, status uint8; bit 0 = cells off the
    board dropped, bit 1 = stopped at a "$" count of 129)."""
    if not (text.is_cuda and offsets.is_cuda) or text.dtype != torch.uint8 or offsets.dtype != torch.int64:
        raise ValueError("text must be a device uint8 tensor, offsets a device int64 tensor")
    n = offsets.numel() - 1
    out = torch.empty((max(n, 0), N), dtype=torch.int64, device=text.device)
    status = torch.empty(max(n, 0), dtype=torch.uint8, device=text.device)
    buf = text if text.numel() else torch.zeros(1, dtype=torch.uint8, device=text.device)
    _check(lib.lifeapi_parse_rle_batch_dev(buf.data_ptr(), offsets.data_ptr(), max(n, 0), out.data_ptr(),
                                           status.data_ptr(), _stream(stream)))
    return out, status


def rle_host(states: np.ndarray, device: int = 0) -> list[str]:
    """Host-pointer ``lifeapi_rle_batch``: size query, then the write."""
    src = _host_u64(states)
    n = src.size // N
    offs = np.zeros(n + 1, dtype=np.uint64)
    _check(lib.lifeapi_rle_batch(src.ctypes.data, n, None, 0, offs.ctypes.data, device))
    text = ctypes.create_string_buffer(max(int(offs[-1]), 1))
    _check(lib.lifeapi_rle_batch(src.ctypes.data, n, text, int(offs[-1]), offs.ctypes.data, device))
    raw = text.raw
    return [raw[int(offs[u]):int(offs[u + 1])].decode() for u in range(n)]


def parse_rle_host(patterns: list[str | bytes], device: int = 0) -> tuple[np.ndarray, np.ndarray]:
    """Host-pointer ``lifeapi_parse_rle_batch``."""
    bs = [p.encode() if isinstance(p, str) else bytes(p) for p in patterns]
    offs = np.zeros(len(bs) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(b) for b in bs])
    blob = b"".join(bs) or b"\0"
    out = np.zeros((len(bs), N), dtype=np.uint64)
    status = np.zeros(len(bs), dtype=np.uint8)
    _check(lib.lifeapi_parse_rle_batch(blob, offs.ctypes.data, len(bs), out.ctypes.data, status.ctypes.data,
                                       device))
    return out, status
