# The host driver of the MSM slot forms (tests/test_slot_form_host.py): msm_finish_host under the sanitizer flags of the Makefile beside
# it ($(SAN)), which this file includes rather than repeats.   make -f slot_form.mk slot_form_host_san
include Makefile
SDEPS = slot_form_host.cpp $(CSRC)/msm_slot.hpp $(CSRC)/g1_host.hpp $(CSRC)/g1.hpp $(CSRC)/endo.hpp $(CSRC)/field.hpp $(CSRC)/constants.hpp
slot_form_host_san: $(SDEPS)
	$(CXX) $(SAN) slot_form_host.cpp -o $@
