// Run-time specialised assembly kernel (jit.cpp).
#pragma once
#include <string>
#include <vector>

namespace mrk {

struct Program;
struct QsSignature;  // forest.hpp: the forest's view signature - the kernels that write the scorer's tile are keyed by it too

// the specialised kernels of a program; each is compiled (and cached on disk) by itself when a batch first needs it
//   JIT_RANK      mrk_jit_rank_cells: the workgroup-per-request assembly of full batches, tables in 4-byte entries
//   JIT_SPLIT     mrk_jit_rank_cells_split: its op-split / sliced form (a handful of requests, few large ones, wide tables)
//   JIT_MATRIX    mrk_jit_rank_matrix: the same writing the row-major f64 matrix; keyed by the program only
//   JIT_ITEMS     mrk_jit_assemble_cells: the item-parallel assembly (requests too large for one workgroup)
//   JIT_ITEMS_RT  mrk_jit_assemble_cells_rt: its persistent form with every threshold table of the forest resident in LDS; exists
//                 only for a forest whose signature is known and whose tables fit (jit_items_rt_applies)
//   JIT_ONE       mrk_jit_rank_one: pre-pass + assembly + forest + ordering of a small request in one launch
//   JIT_SERVE     mrk_jit_rank_serve: the persistent workgroup of the serving queue
//   JIT_UNUSED    no kernel (once the one-launch kernel of full batches): the number stays taken - cache slots and the mask bits
//                 of mrk_config_precompile keep their meaning; a mask with bit 6 compiles nothing for it
//   JIT_PREPASS   mrk_jit_prepass: the pre-pass alone (in front of JIT_ITEMS); keyed by the program only
//   JIT_ONE_WALK, JIT_SERVE_WALK  the one-launch kernel and the persistent workgroup of a forest scored by the tree walk: keyed by
//                 the program and the scorer's precision only - such a forest has no view signature
//   JIT_VALUES    mrk_jit_rank_values: pre-pass + assembly of small requests in one launch, the f64 rows stored straight into
//                 pinned host memory (mrk_values); keyed by the program only
enum { JIT_RANK = 0, JIT_SPLIT = 1, JIT_MATRIX = 2, JIT_ITEMS = 3, JIT_ONE = 4, JIT_SERVE = 5, JIT_UNUSED = 6, JIT_PREPASS = 7, JIT_ITEMS_RT = 8, JIT_ONE_WALK = 9, JIT_SERVE_WALK = 10, JIT_VALUES = 11, JIT_KERNELS = 12, JIT_ALL = -1, JIT_NONE = -2 };
// the translation unit hiprtc compiles for this model's program: the shared device code + the program as constants +
// the kernel `kernel` (JIT_ALL: every kernel - inspection tools)
std::string jit_source(const Program &prog, bool f64, int kernel = JIT_ALL, const QsSignature *sig = nullptr);
// gfx950 code object of `source`; throws StatusError(MRK_ERR_DEVICE) with the compiler log.  No device needed.
std::vector<char> jit_compile(const std::string &source, std::string &log);
// hipFunction_t of kernel `kernel` for (program, scorer precision, forest signature or nullptr), built on first use; nullptr when
// specialisation is switched off (MRK_RANK_JIT=0), while it compiles in the background, or when hiprtc failed (warning on stderr;
// MRK_RANK_JIT=require throws).  The serving queue's kernels wait for the compiler: mrk_serve_start is the warm-up.
void *jit_function(const Program &prog, int kernel, bool f64, const QsSignature *sig);
bool jit_items_rt_applies(const QsSignature *sig);
int jit_precompile(const Program &prog, bool f64, unsigned kernel_mask, const std::string &dir, const QsSignature *sig = nullptr);
void jit_wait(const Program &prog);
std::string jit_loaded_keys(const Program &prog);
void jit_release(Program &prog);

}  // namespace mrk
