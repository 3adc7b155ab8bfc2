// inst.hip — one capacity instance of the team kernels per translation unit (build.py compiles this
// file once per -DMG_INST=i, i < MG_NUM_INST, in parallel, and links the objects with migym.hip).
// With -DMG_CONTACTS_TU the unit holds the instance's contact read-out alone (k_contacts, mg_debug_contacts: tests
// only) -- a code object of its own, so that the shipped instances' code objects are what they are without it.
// With -DMG_LINKFORCE_TU it holds the instance's k_simulate with link forces alone (k_simulate_xf), likewise.
// With -DMG_HEIGHTFIELD_TU it holds the instance's k_simulate on heightfield terrain and that kernel's contact read-out
// alone (k_simulate_hf, k_contacts_hf), likewise.  The four kinds of unit are one table in build.py (`kinds`), and the
// five kernels are wrappers over one body (step_kernels.hpp).
#include "step_kernels.hpp"

#ifndef MG_INST
#error "compile with -DMG_INST=<instance index> (build.py)"
#endif
static_assert(MG_INST >= 0 && MG_INST < MG_NUM_INST, "MG_INST out of range");

namespace mgi {
constexpr InstDesc kI = kInst[MG_INST];
#if defined(MG_LINKFORCE_TU)
static_assert(kI.OBJ == 0 && kI.LAY == 0, "link forces: the objectless instances in the classic layout (build.py)");
template struct RunSimulateXF<kI.T, kI.MN, kI.MC, kI.MG, kI.MP>;
#elif defined(MG_HEIGHTFIELD_TU)
static_assert(kI.OBJ == 0 && kI.LAY == 0, "heightfield: the objectless instances in the classic layout (build.py)");
template struct RunSimulateHF<kI.T, kI.MN, kI.MC, kI.MG, kI.MP>;
template struct RunContactsHF<kI.T, kI.MN, kI.MC, kI.MG, kI.MP>;
#elif defined(MG_CONTACTS_TU)
template struct RunContacts<kI.T, kI.MN, kI.MC, kI.MG, kI.MP, kI.OBJ, kI.LAY>;
#else
template struct BuildTile<kI.T, kI.MN, kI.MC, kI.MG, kI.MP, kI.OBJ, kI.LAY>;
template struct RunSimulate<kI.T, kI.MN, kI.MC, kI.MG, kI.MP, kI.OBJ, kI.LAY>;
template struct RunEnvStep<kI.T, kI.MN, kI.MC, kI.MG, kI.MP, kI.OBJ, kI.LAY>;
template int phase_buf_publish<MG_INST>(unsigned long long*);
#endif
}  // namespace mgi
