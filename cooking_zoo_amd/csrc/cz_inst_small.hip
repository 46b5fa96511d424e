// instantiation unit: one object slot and one grid cell per lane (D <= 64, W*H <= 64), e.g. the 7x7 levels
#include "cz_launch.h"
namespace cz {
Launchers launchers_small() { return Inst<1, 1, true>::launchers(); }
}
