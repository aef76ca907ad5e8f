// the coupled four-state test twin with two controls (cxu is a 4 x 2 block: a transposed read shows)
#define ILQR_COUPLED4_NU 2
#include "user_model_coupled4.hpp"
