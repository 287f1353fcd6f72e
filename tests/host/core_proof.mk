# The host driver of the core-proof layout, transcript and batch digest (tests/test_core_proof_host.py): a plain build and one under the
# sanitizer flags of the Makefile beside it ($(SAN)), which this file includes rather than repeats.
#   make -f core_proof.mk core_proof_host core_proof_host_san
include Makefile
KDEPS = core_proof_host.cpp $(CSRC)/proof_layout.hpp $(CSRC)/fs.hpp $(CSRC)/sha256.hpp $(CSRC)/field.hpp $(CSRC)/constants.hpp
core_proof_host: $(KDEPS)
	$(CXX) -O2 -std=c++17 -w core_proof_host.cpp -o $@
core_proof_host_san: $(KDEPS)
	$(CXX) $(SAN) core_proof_host.cpp -o $@
