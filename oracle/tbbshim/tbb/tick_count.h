/* Serial stand-in: see serial_shim.h (test infrastructure only). */
#include "serial_shim.h"
