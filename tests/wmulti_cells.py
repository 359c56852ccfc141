"""The launch plan of the model-wide weight launches as data (test infrastructure; pure integers, no torch, no GPU).

mhaq_fq_wlayer_fwd_multi and launch_pc_bwd_multi (csrc/fq_pc.hip) pick a kernel instantiation -- a CELL -- from three
integers of the launch: max_row, total_co, nlayers.  Inside the kernel every row then takes one of three BODIES.  This module
restates those host rules (multi_threads, multi_reg_nv, the per128 rule of the forward, the 9 x 1024 rule of whole-tensor
launches) and the per-row choice, and holds the case table of tests/test_gpu_weight_multi_cells.py: small plans whose
DEFINING layer sets max_row on either side of every threshold, each with the other row bodies its cell can hold.

Cell names: "F<NV>x<threads>" / "B<NV>x<threads>" for pc_fwd_multi_reg_kernel<NV,TB> / pc_bwd_multi_reg_kernel<M,NV,TB>,
"Fgen1024" / "Bgen1024" for pc_fwd_multi_kernel / pc_bwd_multi_kernel<M> at 1024 threads.
Row bodies: "reg" (aligned, a whole number of float4, fits NV * TB float4), "unstaged" (aligned but too long -- in the
generic kernels: every aligned row), "dword" (row % 4 != 0, or the layer starts off the 16-byte grid of its slab).

A layer is (kind, qscheme, shape): kind "conv" -> NoisyConv2d(shape[1], shape[0], shape[2], bias=False), "linear" ->
NoisyLinear(shape[1], shape[0]); qscheme "pc" (PER_CHANNEL: co = shape[0] rows) or "pt" (PER_TENSOR: ONE row, the whole
tensor, multi.py).  Weights and their slabs come from the allocator, 256-byte aligned: alignment is a matter of the element
offset alone."""
from collections import namedtuple

K_BLOCK = 256                 # fq_common.hpp kBlock
K_WIDE = 64 * 16              # 64 * kMaxWaves: the workgroup of whole-tensor launches
WHOLE_MIN_ROW = 8192          # multi_threads()
PT_MAX_ELEMS = 64 * 1024      # mhaq_fq_wlayer_pt_max_elements(): the longest PER_TENSOR layer that rides the plan

FWD_CELLS = ("F2x128", "F4x128", "F9x128", "F8x256", "F9x1024", "Fgen1024")
BWD_CELLS = ("B2x256", "B4x256", "B5x256", "B8x256", "B9x1024", "Bgen1024")
# instantiated by the forward's launch code, selected by no max_row (tests/test_wmulti_cells_cpu.py)
FWD_UNREACHABLE = ("F2x256", "F4x256")
# cells no test selected before tests/test_gpu_weight_multi_cells.py: the stray-write checks run on these
NEW_CELLS = ("F4x128", "B4x256", "Fgen1024", "Bgen1024")


def _items(max_row):
    return (max_row + 3) // 4


def whole_tensor(max_row, total_co, nlayers):
    """multi_threads() == 1024: a launch whose rows are whole tensors."""
    return max_row >= WHOLE_MIN_ROW and total_co <= 2 * nlayers


def multi_reg_nv(max_row, backward):
    per = (_items(max_row) + K_BLOCK - 1) // K_BLOCK
    return 2 if per <= 2 else (4 if per <= 4 else (5 if (per <= 5 and backward) else 8))


def fwd_cell(max_row, total_co, nlayers):
    if not whole_tensor(max_row, total_co, nlayers):
        per128 = (_items(max_row) + 127) // 128
        if per128 <= 9:
            return "F2x128" if per128 <= 2 else ("F4x128" if per128 <= 4 else "F9x128")
        return "F%dx256" % multi_reg_nv(max_row, False)
    return "F9x1024" if _items(max_row) <= 9 * K_WIDE else "Fgen1024"


def bwd_cell(max_row, total_co, nlayers):
    """total_co / nlayers of the LAUNCH: a group's own for mhaq_fq_wlayer_bwd_group."""
    if not whole_tensor(max_row, total_co, nlayers):
        return "B%dx256" % multi_reg_nv(max_row, True)
    return "B9x1024" if _items(max_row) <= 9 * K_WIDE else "Bgen1024"


def cell_capacity(cell):
    """float4 a register-resident row of the cell may have (NV * TB); 0 for the generic kernels."""
    if "gen" in cell:
        return 0
    nv, tb = cell[1:].split("x")
    return int(nv) * int(tb)


def row_body(row, aligned, cell):
    """aligned: the layer's element offset in the slab is a multiple of 4."""
    if row % 4 or not aligned:
        return "dword"
    return "reg" if (row >> 2) <= cell_capacity(cell) else "unstaged"


def reachable_bodies(cell):
    """The row bodies a launch of `cell` can run: the cell is chosen from the longest row, so an aligned row that overflows
    NV * TB exists only where the cell is open-ended (the 8 x 256 cells) and in the generic kernels, which have no
    register body."""
    if "gen" in cell:
        return ("unstaged", "dword")
    if cell in ("F8x256", "B8x256"):
        return ("reg", "unstaged", "dword")
    return ("reg", "dword")


# ---------------------------------------------------------------------------------------------------------- plans
def layer_co_row(layer):
    kind, qscheme, shape = layer
    n = 1
    for d in shape:
        n *= d
    co = shape[0] if qscheme == "pc" else 1
    return co, n // co


class Plan(namedtuple("Plan", "co row elem_off chan_off total_co total_elems max_row nlayers")):
    """What multi.py::MultiTensorWeightQuant derives from its layers."""

    @classmethod
    def of(cls, layers):
        co, row, eo, cho, e, c = [], [], [], [], 0, 0
        for layer in layers:
            k, r = layer_co_row(layer)
            co.append(k)
            row.append(r)
            eo.append(e)
            cho.append(c)
            e += k * r
            c += k
        return cls(tuple(co), tuple(row), tuple(eo), tuple(cho), c, e, max(row), len(layers))

    def cells(self, first=0, last=None):
        """(forward cell of the model-wide launch, backward cell of the group [first, last))."""
        last = self.nlayers if last is None else last
        return (fwd_cell(self.max_row, self.total_co, self.nlayers),
                bwd_cell(max(self.row[first:last]), sum(self.co[first:last]), last - first))

    def bodies(self, first=0, last=None):
        """Per layer of the group: (forward body, backward body).  The forward's offsets count from the start of the
        model, the group's from its first layer."""
        last = self.nlayers if last is None else last
        f, b = self.cells(first, last)
        return [(row_body(self.row[i], self.elem_off[i] % 4 == 0, f),
                 row_body(self.row[i], (self.elem_off[i] - self.elem_off[first]) % 4 == 0, b))
                for i in range(first, last)]


def _pc(row, co):
    return ("linear", "pc", (co, row))


def _pt(row):
    assert row % 4 == 0 and row <= PT_MAX_ELEMS
    return ("linear", "pt", (4, row // 4))         # NoisyLinear(in, 4): any row length that is a multiple of 4


SHORT = ("conv", "pc", (3, 4, 3, 3))               # 36-float rows, aligned


def _odd(co):
    return ("conv", "pc", (co, 3, 3, 3))           # 27-float rows: the dword body, and 27 * co floats shift what follows


Case = namedtuple("Case", "name layers defining long_rows channels_last per_tensor")


def _case(name, head, tail, defining=0, long_rows=False, channels_last=False, odd_co=None):
    """head + a 27-float layer + tail: the first layer of `tail` has an aligned length and must start off the 16-byte grid;
    the 27-float layer's channel count (2-5) is chosen so that it does unless `odd_co` fixes it."""
    for co in ((odd_co,) if odd_co else (3, 2, 5, 4)):
        layers = tuple(head) + (_odd(co),) + tuple(tail)
        p = Plan.of(layers)
        if p.elem_off[len(head) + 1] % 4:
            break
    else:
        raise AssertionError(name)
    return Case(name, layers, defining, long_rows, channels_last, any(l[1] == "pt" for l in layers))


def _pc_case(row, **kw):
    """Per-channel plan whose defining layer [3, row] comes first (offset 0), then a short aligned layer, the 27-float layer
    and a [2, row] layer off the grid."""
    return _case("pc%d" % row, [_pc(row, 3), SHORT], [_pc(row, 2)], **kw)


def _pt_case(row, short_co=3, name=None, **kw):
    """Whole-tensor plan: the defining PER_TENSOR layer of `row` floats, a short per-channel layer of `short_co` channels, the
    27-float layer (3 channels) and a PER_TENSOR 8x16x3x3 convolution off the grid: total_co = 5 + short_co over 4 layers."""
    return _case(name or "pt%d" % row, [_pt(row), ("conv", "pc", (short_co, 4, 3, 3))],
                 [("conv", "pt", (8, 16, 3, 3))], odd_co=3, **kw)


CASES = (
    # forward per-channel thresholds 1024 | 1028, 2048 | 2052, 4608 | 4612; backward 2048 | 2052, 4096 | 4100, 5120 | 5124
    _pc_case(1024),
    _pc_case(1028),
    # a maximum that is no multiple of 4: the dword layer sets the cell (ceil(1025 / 4) = 257 float4 -> NV 4 at 128 threads),
    # the aligned [3, 1024] layer beside it runs that cell's register body
    _case("pc1025", [_pc(1024, 3), SHORT, _pc(1025, 3)], [_pc(1024, 2)], defining=2),
    _pc_case(2048),
    _pc_case(2052),
    _pc_case(4096),
    _pc_case(4100),
    _pc_case(4608, channels_last=True),
    _pc_case(4612),
    _pc_case(5120),
    _pc_case(5124),
    # beyond 8 float4 per thread at 256 threads: the defining rows take the unstaged body, the [2, 8192] layer fills the
    # register body to its last float4 (long_rows=True: a trainer's default plan leaves such layers out, multi.py)
    _case("pc8196", [_pc(8196, 3), _pc(8192, 2), SHORT], [_pc(8196, 2)], long_rows=True),
    # whole-tensor launches: max_row >= 8192 and total_co <= 2 * nlayers
    _pt_case(8188),
    _pt_case(8192),                                          # total_co = 8 = 2 * nlayers
    _pt_case(8192, short_co=4, name="pt8192_co9"),           # total_co = 9 = 2 * nlayers + 1: back to 256 threads
    _pt_case(36864, channels_last=True),
    _pt_case(36868),
    _pt_case(65532, channels_last=True),
    _pt_case(65536),                                         # the longest PER_TENSOR layer the plan takes
    # per-channel layers of two channels each are "whole tensors" to the rule as well (total_co = 2 * nlayers): the only
    # way AEWGS reaches the 1024-thread kernels
    _case("pcw36864", [_pc(36864, 2), ("conv", "pc", (2, 4, 3, 3))], [_pc(1152, 2)], odd_co=2, long_rows=True),
    _case("pcw36868", [_pc(36868, 2), ("conv", "pc", (2, 4, 3, 3))], [_pc(1152, 2)], odd_co=2, long_rows=True),
)
CASE = {c.name: c for c in CASES}

# (kind, below, above): the defining rows on the two sides of a threshold, 4 floats apart
THRESHOLDS = (
    ("fwd", "pc1024", "pc1028"), ("fwd", "pc2048", "pc2052"), ("fwd", "pc4608", "pc4612"),
    ("bwd", "pc2048", "pc2052"), ("bwd", "pc4096", "pc4100"), ("bwd", "pc5120", "pc5124"),
    ("both", "pt8188", "pt8192"), ("both", "pt36864", "pt36868"),
)
# the top of the range: both sides in the generic kernels, 65536 the last length a PER_TENSOR layer may have in a plan
TOP_PAIR = ("pt65532", "pt65536")
# total_co on the two sides of 2 * nlayers at the same rows
CO_PAIR = ("pt8192", "pt8192_co9")


def estimators(case):
    """AEWGS keeps PER_TENSOR layers out of the plan (multi.py: its statistics are per position for a [1]-shaped scale)."""
    return ("STE", "LSQ", "EWGS") if case.per_tensor else ("STE", "LSQ", "EWGS", "AEWGS")


# ------------------------------------------------------------------------------------- the plans of the earlier tests
def _convs(shapes, q="pc"):
    return tuple(("conv", q, s) for s in shapes)


_GROUPS_SHAPES = ((16, 16, 3, 3), (32, 16, 3, 3), (12, 12, 3, 3), (10, 5, 1, 1), (64, 32, 3, 3), (512, 512, 3, 3),
                  (24, 50, 3, 3))
_PT_SHAPES = ((16, 16, 3, 3), (32, 16, 3, 3), (12, 12, 3, 3), (10, 5, 1, 1), (64, 64, 3, 3), (24, 50, 3, 3))
_LONG = (("conv", "pc", (8, 3, 3, 3)), ("conv", "pc", (24, 64, 3, 3)), _pc(16384, 6), ("conv", "pc", (12, 512, 3, 3)),
         _pc(40004, 3), ("conv", "pc", (16, 128, 3, 3)))

# (where, layers, backward groups [first, last), forward cell, backward cell per group): the model-wide plans the suite
# ran before this table, their cells written out by hand from the shape tables of those tests
EXISTING_PLANS = (
    ("test_gpu_weight_groups.py::test_grouped_backward_equals_per_layer_ops", _convs(_GROUPS_SHAPES), ((5, 7), (1, 5)),
     "F9x128", ("B5x256", "B2x256")),
    ("test_gpu_weight_groups.py::test_per_tensor_layers_ride_the_model_wide_launch_as_one_channel",
     _convs(_PT_SHAPES, "pt") + _convs([(6, 8, 3, 3)]), ((0, 7),), "F9x1024", ("B9x1024",)),
    ("test_gpu_weight_groups.py::test_noisy_linear_layers_take_part_in_the_model_wide_launches",
     (_pc(64, 10), ("conv", "pc", (6, 8, 3, 3)), ("linear", "pt", (7, 33))), ((0, 3),), "F2x128", ("B2x256",)),
    ("test_gpu_weight_groups.py::test_models_on_both_sides_of_64_layers_find_their_rows[97]",
     tuple(("conv", "pc", (2 + (i * 7) % 11, 4 + 4 * (i % 5), 3, 3) if i % 3 else (3 + i % 4, 8 + 4 * (i % 3), 1, 1))
           for i in range(97)), ((0, 97),), "F2x128", ("B2x256",)),
    ("test_gpu_weight_groups.py::test_a_per_channel_model_with_one_long_row_layer_keeps_the_per_layer_bits", _LONG,
     ((0, 6),), "F8x256", ("B8x256",)),
    ("test_gpu_weight_groups.py::test_default_plan_next_to_excluded_long_row_layers_keeps_the_per_layer_bits",
     _convs([(24, 64, 3, 3), (12, 512, 3, 3), (16, 128, 3, 3)]), ((0, 3),), "F9x128", ("B5x256",)),
    ("test_gpu_weight_groups.py::test_descriptor_pool_recycles_its_entries_without_mixing_tables",
     _convs([(8, 4, 3, 3), (6, 8, 3, 3), (5, 6, 3, 3)]), ((0, 3),), "F2x128", ("B2x256",)),
    ("test_gpu_fused_layers.py::test_multi_tensor_weight_quant_equals_per_layer_ops",
     _convs([(16, 16, 3, 3), (32, 16, 3, 3), (32, 32, 3, 3), (64, 32, 3, 3), (12, 12, 3, 3), (512, 512, 3, 3)]), ((0, 6),),
     "F9x128", ("B5x256",)),
    ("test_gpu_row_extremes.py::test_grouped_launch_equals_per_layer_on_planted_extremes",
     _convs([(16, 128, 3, 3), (8, 256, 3, 3), (4, 512, 3, 3), (4, 64, 1, 1)]), ((0, 4),), "F9x128", ("B5x256",)),
    # the two multi fuzzers draw co 1-19, ci 1-17, k in {1, 3, 5}: the longest row they can draw
    ("test_gpu_fuzz.py::test_fuzz_multi_tensor_mixed_alignment / test_fuzz_grouped_weight_backward (longest row)",
     _convs([(19, 17, 5, 5), (19, 17, 3, 3), (19, 17, 1, 1)]), ((0, 3),), "F2x128", ("B2x256",)),
)
